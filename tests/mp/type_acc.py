"""One-sided accumulate between ranks: Accumulate / Get_accumulate / Fetch_and_op on basic and
derived target types in one type_accumulate launch under one target lock (Window::accumulate_plan
over csrc/kernels/type_acc.hip), on 2 ranks under torch.distributed.run. T_DEVICE=cuda: the ranks
share the box's GPU and windows / buffers are HBM; otherwise host shm windows and the host twin.

Every comparison is bitwise against a per-element oracle built from the type map's definition
and comb(target, origin) in numpy / torch, over the target's WHOLE window, sentinels included.
Each case prints ``OK <case>`` on rank 0. Cases (T_CASES, comma separated): ops, compat, atomic,
fetch, bounds. `compat` also runs under MPIT_DTYPE_KERNEL=0 (the per-run axpby path) and prints
the bytes it produced as ``RESULT compat <hex>`` for the caller to compare between the two."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import mpit_amd as mp
from mpit_amd import datatypes as dt
from mpit_amd import mpiT
from mpit_amd.comm import COMM_WORLD

mp.Init()
W = COMM_WORLD()
r, n = W.Get_rank(), W.Get_size()
assert n == 2
peer = 1 - r
on_gpu = os.environ.get("T_DEVICE", "cpu") == "cuda"
dev = mp.runtime.device() if on_gpu else torch.device("cpu")
cases = os.environ.get("T_CASES", "ops,compat,atomic,fetch,bounds").split(",")
SENT = 0xA5
WIN_BYTES = 4096
KINDS = {"i32": (torch.int32, dt.INT), "f32": (torch.float32, dt.FLOAT), "bf16": (torch.bfloat16, dt.BFLOAT16)}


def ok(name):
    W.Barrier()
    if r == 0:
        print("OK", name, flush=True)


def type_index(t, count):
    idx = []
    for i in range(count):
        for d, b in t.typemap:
            idx.extend(range(i * t.extent + d, i * t.extent + d + dt._BASIC[b][0]))
    return np.array(idx, dtype=np.int64)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def sync_dev():
    if on_gpu:
        torch.cuda.synchronize()


def as_bytes(x):
    return x.contiguous().view(torch.uint8).numpy()


def values(kind, ne, seed):
    """ne host elements: full-range integers; eighths with +-inf and (fp32) NaN among them."""
    rng = np.random.default_rng(seed)
    tdt = KINDS[kind][0]
    if kind == "i32":
        v = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, ne, dtype=np.int64)).to(tdt)
        v[::5] = 0
        return v
    v = torch.from_numpy(rng.integers(-64, 65, ne) / 8.0).to(tdt)
    v[seed % 7] = float("inf")
    v[7 + seed % 5] = float("-inf")  # +inf lives in [0, 7), -inf in [7, 12): SUM never adds one to the other
    if kind == "f32":
        v[12 + seed % 3] = float("nan")
    return v


def comb(op, t, o):
    """comb(target, origin) as csrc/kernels/kernels.h defines it, for the ops used here."""
    if t.dtype == torch.int32:
        a, b = t.numpy(), o.numpy()
        if op is mpiT.MAX:
            res = np.where(a > b, a, b)
        elif op is mpiT.PROD:
            res = (a.view(np.uint32) * b.view(np.uint32)).view(np.int32)
        elif op is mpiT.BAND:
            res = a & b
        else:
            res = (a.view(np.uint32) + b.view(np.uint32)).view(np.int32)
        return torch.from_numpy(np.ascontiguousarray(res))
    a, b = t.float(), o.float()
    if op is mpiT.MIN:
        res = torch.where(torch.isnan(a), a, torch.where(torch.isnan(b), b, torch.where(a < b, a, b)))
    else:
        res = a + b
        assert not bool(torch.isnan(res).any())  # see values()
    return res.to(t.dtype)


def new_window(init=None):
    win = mpiT.Win_create(torch.full((WIN_BYTES,), SENT, dtype=torch.uint8, device=dev), comm=W)
    win.tensor.fill_(SENT)  # a host window is a shm copy: fill the exposed memory itself
    if init is not None:
        win.tensor.copy_(to_dev(init))
    sync_dev()
    mpiT.Win_fence(0, win)
    return win


def window_image(tidx, vals):
    img = np.full(WIN_BYTES, SENT, dtype=np.uint8)
    img[tidx] = as_bytes(vals)
    return img


def origin_for(kind, ne, derived, seed):
    """(origin tensor, count, datatype, the elements it carries) with seeded values."""
    tdt, basic = KINDS[kind]
    carried = values(kind, ne, seed)
    if not derived:
        return carried.to(dev), ne, basic, carried
    org = dt.Type_vector(4, 1, 3, basic)
    assert ne % 4 == 0
    es = carried.element_size()
    idx = type_index(org, ne // 4)
    host = np.full(int(idx.max()) + 1, SENT, dtype=np.uint8)
    host[idx] = as_bytes(carried)
    return to_dev(host).view(tdt), ne // 4, org, carried


VEC_I = dt.Type_vector(64, 2, 5, dt.INT)  # 64 runs of 8 bytes every 20
VEC_B = dt.Type_vector(64, 2, 5, dt.BFLOAT16)
IRR_F = dt.Type_create_hindexed([2, 1, 6, 3], [4, 16, 40, 80], dt.FLOAT)  # irregular, lengths and offsets in fours
IRR_I = dt.Type_create_hindexed([2, 1, 6, 3], [4, 16, 40, 80], dt.INT)

if "ops" in cases:
    assert dt.kernel_enabled()
    combos = [("i32", VEC_I, 1, 12, mpiT.MAX), ("i32", VEC_I, 1, 12, mpiT.PROD), ("i32", VEC_I, 1, 12, mpiT.BAND),
              ("i32", IRR_I, 8, 16, mpiT.BAND), ("f32", IRR_F, 8, 16, mpiT.MIN), ("bf16", VEC_B, 1, 6, mpiT.SUM)]
    for k, (kind, typ, cnt, disp, op) in enumerate(combos):
        for derived in (False, True):
            tidx = type_index(typ, cnt) + disp
            ne = len(tidx) // KINDS[kind][0].itemsize
            mine = values(kind, ne, 100 + 10 * k + r)  # what my window's target elements hold
            win = new_window(window_image(tidx, mine))
            org, ocnt, otyp, _ = origin_for(kind, ne, derived, 200 + 10 * k + r + 2 * derived)
            before = dict(dt.COUNTERS)
            assert mpiT.Accumulate(org, ocnt, otyp, peer, disp, cnt, typ, op, win) == mpiT.SUCCESS
            assert dt.COUNTERS["rma_acc_kernel"] == before["rma_acc_kernel"] + 1, dt.COUNTERS
            assert dt.COUNTERS["rma_acc_runs"] == before["rma_acc_runs"] == 0
            mpiT.Win_fence(0, win)
            # what the peer accumulated onto MY window: its origin elements, regenerated from its seed
            _, _, _, theirs = origin_for(kind, ne, derived, 200 + 10 * k + peer + 2 * derived)
            want = window_image(tidx, comb(op, mine, theirs))
            got = win.tensor.cpu().numpy()
            assert np.array_equal(got, want), (kind, typ, op, derived, np.flatnonzero(got != want)[:8])
            mpiT.Win_fence(0, win)
            mpiT.Win_free(win)
    # the object API: a basic contiguous target, an op and a type that are new
    win = mp.Win.Allocate(64, torch.int64, W, device=on_gpu)
    win.tensor.fill_(5)
    sync_dev()
    win.Fence()
    before = dict(dt.COUNTERS)
    win.Accumulate(torch.arange(8, dtype=torch.int64, device=dev), peer, 3, op=mpiT.MAX)
    win.Raccumulate(torch.full((2,), 6, dtype=torch.int64, device=dev), peer, 20, op=mpiT.BXOR).Wait()
    assert dt.COUNTERS["rma_acc_kernel"] == before["rma_acc_kernel"] + 2 and dt.COUNTERS["rma_acc_runs"] == 0
    win.Fence()
    want = torch.full((64,), 5, dtype=torch.int64)
    want[3:11] = torch.tensor([5, 5, 5, 5, 5, 5, 6, 7])
    want[20:22] = 3
    assert torch.equal(win.tensor.cpu(), want), win.tensor.cpu()
    # a float bitwise op and an element type outside the seven: TypeError naming both, nothing moves
    for org, bad_op, names in ((torch.ones(4, device=dev), mpiT.BAND, ("BAND", "float32")),
                               (torch.ones(4, dtype=torch.int16, device=dev), mpiT.SUM, ("SUM", "int16"))):
        fw = mp.Win.Allocate(4, org.dtype, W, device=on_gpu)
        fw.Fence()
        for call in (lambda: fw.Accumulate(org, peer, 0, op=bad_op),
                     lambda: mpiT.Accumulate(org, 4, None, peer, 0, 4, None, bad_op, fw)):
            try:
                call()
                raise AssertionError("unsupported (op, type) accepted")
            except TypeError as e:
                assert all(s in str(e) for s in names), e
        fw.Fence()
        assert not bool(fw.tensor.any())
        fw.Lock(peer)  # and no lock is left behind
        fw.Unlock(peer)
        fw.Fence()
        fw.Free()
    win.Free()
    ok("ops")

if "compat" in cases:
    # the Accumulate lines of tests/mp/api_suite.py: the same values on either path
    kernel = dt.kernel_enabled()
    before = dict(dt.COUNTERS)
    acc = mp.Win.Allocate(4, torch.float32, W, device=on_gpu)
    acc.Fence()
    acc.Accumulate(torch.ones(4, device=dev), 0, 0)
    acc.Fence()
    if r == 0:
        assert acc.tensor.tolist() == [float(n)] * 4
    vt = mpiT.Type_commit(mpiT.Type_vector(3, 1, 2, mpiT.FLOAT))
    dw = mpiT.Win_create(torch.zeros(8, device=dev), comm=W)
    dw.tensor.zero_()
    sync_dev()
    mpiT.Win_fence(0, dw)
    src = torch.tensor([r + 1.0, r + 2.0, r + 3.0], device=dev)
    assert mpiT.Put(src, 3, mpiT.FLOAT, (r + 1) % n, 1, 1, vt, dw) == mpiT.SUCCESS
    mpiT.Win_fence(0, dw)
    assert mpiT.Accumulate(torch.ones(3, device=dev), 3, mpiT.FLOAT, 0, 1, 1, vt, mpiT.SUM, dw) == mpiT.SUCCESS
    mpiT.Win_fence(0, dw)
    if r == 0:
        q = n - 1
        assert dw.tensor.tolist() == [0.0, q + 1.0 + n, 0.0, q + 2.0 + n, 0.0, q + 3.0 + n, 0.0, 0.0], dw.tensor.tolist()
    # REPLACE and a bf16 SUM, which both paths have as well
    bw = mp.Win.Allocate(6, torch.bfloat16, W, device=on_gpu)
    bw.tensor.fill_(1.0)
    sync_dev()
    bw.Fence()
    if r == 1:
        bw.Accumulate(torch.tensor([0.00390625, 2.0], dtype=torch.bfloat16, device=dev), 0, 1)
        bw.Accumulate(torch.tensor([7.0], dtype=torch.bfloat16, device=dev), 0, 4, op=mpiT.REPLACE)
    bw.Fence()
    if r == 0:
        assert bw.tensor.tolist() == [1.0, 1.0, 3.0, 1.0, 7.0, 1.0], bw.tensor.tolist()  # 1 + 2^-8 ties to even
    d = {k: dt.COUNTERS[k] - before[k] for k in dt.COUNTERS}
    calls = 2 + (2 if r == 1 else 0)
    if kernel:
        assert d["rma_acc_kernel"] == calls and d["rma_acc_runs"] == 0, d
    else:
        assert d["rma_acc_kernel"] == 0 and d["rma_acc_runs"] == calls + 2, d  # the vector target is 3 runs
        # and what is new stays refused exactly as before the kernel existed
        iw = mp.Win.Allocate(4, torch.int32, W, device=on_gpu)
        iw.Fence()
        for call, exc, text in (
                (lambda: acc.Accumulate(torch.ones(4, device=dev), 0, 0, op=mpiT.MAX), ValueError, "Accumulate supports SUM and REPLACE"),
                (lambda: mpiT.Accumulate(torch.ones(3, device=dev), 3, mpiT.FLOAT, 0, 1, 1, vt, mpiT.MAX, dw), ValueError,
                 "Accumulate supports SUM and REPLACE"),
                (lambda: iw.Accumulate(torch.ones(4, dtype=torch.int32, device=dev), 0, 0), TypeError,
                 "Accumulate supports float32 / bfloat16"),
                (lambda: mpiT.Accumulate(torch.ones(4, dtype=torch.int32, device=dev), 4, mpiT.INT, 0, 0, 4, mpiT.INT,
                                         mpiT.SUM, iw), TypeError, "fp32 / bf16 elements of one type on both sides")):
            try:
                call()
                raise AssertionError("accepted without the kernel")
            except exc as e:
                assert text in str(e), e
        try:
            mpiT.Fetch_and_op(torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                              mpiT.INT, 0, 0, mpiT.SUM, iw)
            raise AssertionError("Fetch_and_op without the kernel accepted")
        except ValueError as e:
            assert "MPIT_DTYPE_KERNEL" in str(e), e
        iw.Fence()
        iw.Free()
    acc.Fence()
    if r == 0:
        blob = b"".join(as_bytes(t.cpu()).tobytes() for t in (acc.tensor, dw.tensor, bw.tensor))
        print("RESULT compat", blob.hex(), flush=True)
    for w in (acc, dw, bw):
        w.Free()
    ok("compat")

if "atomic" in cases:
    # both ranks, in one fence epoch, 50 accumulates each onto the same 1,024 elements of rank 0
    N, REPS = 1024, 50
    iw = mp.Win.Allocate(N, torch.int32, W, device=on_gpu)
    fw = mp.Win.Allocate(N, torch.float32, W, device=on_gpu)
    iw.Fence()
    fw.Fence()
    lane = torch.arange(N, dtype=torch.int64)
    total_i = torch.zeros(N, dtype=torch.int64)
    total_f = torch.zeros(N, dtype=torch.float64)
    for rank in range(n):
        for k in range(REPS):
            total_i += 0x61000000 + 977 * k + rank + lane  # wraps many times in 32 bits
            total_f += 3 * k + rank + (lane % 7)  # small integers: exact and order-free in fp32
    before = dt.COUNTERS["rma_acc_kernel"]
    for k in range(REPS):
        oi = (0x61000000 + 977 * k + r + lane).to(torch.int32).to(dev)
        of = (3 * k + r + (lane % 7)).to(torch.float32).to(dev)
        if k & 1:
            iw.Accumulate(oi, 0, 0, op=mpiT.SUM)
            fw.Accumulate(of, 0, 0)
        else:
            mpiT.Accumulate(oi, N, mpiT.INT, 0, 0, N, mpiT.INT, mpiT.SUM, iw)
            mpiT.Accumulate(of, N, mpiT.FLOAT, 0, 0, N, mpiT.FLOAT, mpiT.SUM, fw)
    assert dt.COUNTERS["rma_acc_kernel"] == before + 2 * REPS
    iw.Fence()
    fw.Fence()
    if r == 0:
        want_i = (total_i & 0xFFFFFFFF).to(torch.int64)
        got_i = iw.tensor.cpu().to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(got_i, want_i), (got_i[:4], want_i[:4])
        assert float(total_f.max()) < 2 ** 24 and torch.equal(fw.tensor.cpu().double(), total_f)
    iw.Fence()
    iw.Free()
    fw.Free()
    ok("atomic")

if "fetch" in cases:
    # a ticket counter on rank 0: every ticket is drawn exactly once
    cw = mp.Win.Allocate(2, torch.int64, W, device=on_gpu)
    cw.Fence()
    one = torch.ones(1, dtype=torch.int64, device=dev)
    got = torch.full((3,), -1, dtype=torch.int64, device=dev)
    drawn = []
    for k in range(100):
        if k & 1:
            assert mpiT.Fetch_and_op(one, got[1:2], mpiT.LONG, 0, 0, mpiT.SUM, cw) == mpiT.SUCCESS
        else:
            cw.Fetch_and_op(one, got[1:2], 0, 0, op=mpiT.SUM)
        drawn.append(int(got[1]))  # complete on return
    assert got[0] == -1 and got[2] == -1
    every = W.allgather_obj(drawn)
    assert sorted(x for part in every for x in part) == list(range(200)), every
    assert drawn == sorted(drawn)
    cw.Fence()
    if r == 0:
        assert cw.tensor.tolist() == [200, 0]
    # NO_OP without an origin: an atomic read
    cw.Rget_accumulate(None, got[1:2], 0, 0, op=mpiT.NO_OP).Wait()
    assert int(got[1]) == 200
    cw.Fence()
    cw.Free()
    # Get_accumulate with NO_OP: the peer's window, bit for bit, and not a byte of it changed
    image = np.random.default_rng(50 + r).integers(0, 256, WIN_BYTES, dtype=np.uint8)
    theirs = np.random.default_rng(50 + peer).integers(0, 256, WIN_BYTES, dtype=np.uint8)
    win = new_window(image)
    res = torch.full((WIN_BYTES // 4 + 2,), -3.0, device=dev)
    before = dt.COUNTERS["rma_acc_kernel"]
    assert mpiT.Get_accumulate(None, 0, None, res[1:-1], WIN_BYTES // 4, mpiT.FLOAT, peer, 0, WIN_BYTES // 4, mpiT.FLOAT,
                               mpiT.NO_OP, win) == mpiT.SUCCESS
    assert dt.COUNTERS["rma_acc_kernel"] == before + 1
    assert np.array_equal(as_bytes(res[1:-1].cpu()), theirs) and res[0] == -3.0 and res[-1] == -3.0
    mpiT.Win_fence(0, win)
    assert np.array_equal(win.tensor.cpu().numpy(), image)
    mpiT.Win_fence(0, win)
    mpiT.Win_free(win)
    # a derived result type: the fetched elements land where the type says, sentinels elsewhere
    disp = 12
    tidx = type_index(VEC_I, 1) + disp
    ne = len(tidx) // 4
    mine = values("i32", ne, 300 + r)
    win = new_window(window_image(tidx, mine))
    org, ocnt, otyp, _ = origin_for("i32", ne, False, 400 + r)
    rtyp = dt.Type_vector(4, 1, 3, dt.INT)
    ridx = type_index(rtyp, ne // 4)
    result = to_dev(np.full(int(ridx.max()) + 1 + 8, SENT, dtype=np.uint8)).view(torch.int32)
    assert mpiT.Get_accumulate(org, ocnt, otyp, result, ne // 4, rtyp, peer, disp, 1, VEC_I, mpiT.SUM, win) == mpiT.SUCCESS
    want_r = np.full(result.numel() * 4, SENT, dtype=np.uint8)
    want_r[ridx] = as_bytes(values("i32", ne, 300 + peer))  # what the peer's window held
    assert np.array_equal(as_bytes(result.cpu()), want_r)
    mpiT.Win_fence(0, win)
    want = window_image(tidx, comb(mpiT.SUM, mine, values("i32", ne, 400 + peer)))
    assert np.array_equal(win.tensor.cpu().numpy(), want)
    mpiT.Win_fence(0, win)
    mpiT.Win_free(win)
    ok("fetch")

if "bounds" in cases:
    win = new_window()
    ne = VEC_I.Get_size() // 4
    src = torch.ones(ne, dtype=torch.int32, device=dev)
    res = torch.zeros(ne, dtype=torch.int32, device=dev)
    for call in (lambda: mpiT.Accumulate(src, ne, dt.INT, peer, WIN_BYTES - 100, 1, VEC_I, mpiT.MAX, win),
                 lambda: mpiT.Accumulate(src, ne, dt.INT, peer, WIN_BYTES - 4 * ne + 4, ne, dt.INT, mpiT.SUM, win),
                 lambda: mpiT.Get_accumulate(src, ne, dt.INT, res, ne, dt.INT, peer, WIN_BYTES - 100, 1, VEC_I, mpiT.SUM, win),
                 lambda: mpiT.Fetch_and_op(src[:1], res[:1], dt.INT, peer, WIN_BYTES, mpiT.SUM, win)):
        try:  # a span that leaves the window is refused on the host: nothing launched, no lock kept
            call()
            raise AssertionError("accumulate outside the window accepted")
        except IndexError:
            pass
    assert not bool(res.any())
    mpiT.Win_fence(0, win)
    assert bool((win.tensor == SENT).all())
    mpiT.Win_lock(mpiT.LOCK_EXCLUSIVE, peer, 0, win)  # the lock is free
    mpiT.Win_unlock(peer, win)
    mpiT.Win_fence(0, win)
    mpiT.Win_free(win)
    ok("bounds")

W.Barrier()
if r == 0:
    print("ALL_DONE", flush=True)
mp.Finalize()
