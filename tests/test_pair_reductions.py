"""MAXLOC / MINLOC as pair reductions: the window all-reduce, the window collectives and the
one-sided accumulate on (value, index) pairs, interleaved in one dtype or laid out as FLOAT_INT /
DOUBLE_INT / LONG_INT (csrc/kernels/peer_ops.h, comm.py _pair_bind, window.py). The multi-rank
script is tests/mp/pair_reductions.py: bitwise against the CPU fold of the gathered inputs, the
window paths counted in ar_stats / coll_stats, the point-to-point tree giving the same bytes. The
kernels alone are in tests/test_pair_kernels.py."""
import pytest
import torch

from mp_util import run_ranks

ENV = {"MPIT_AR_STAGE_MB": "0.0625"}  # 64 KiB staging window: the staged paths run in several pieces
CPU = {"MPIT_CPU_ONLY": "1", **ENV}
GPU = {"T_DEVICE": "cuda", **ENV}
ALL = ["allreduce", "rooted", "rs", "scan", "facade", "onesided", "errors", "k1"]


def _cases(out, names):
    for c in names:
        assert f"OK {c}" in out, (c, out[-3000:])
    assert "ALL_DONE" in out


# ------------------------------------------------------------------ one process
def test_loc_folds_k_pairs_of_every_layout():
    """The fallback of the point-to-point paths: flat buffers of k pairs, struct pairs through
    typed views of their bytes, the result one of the operand pairs with every byte of it."""
    import numpy as np

    from mpit_amd import comm as C
    from mpit_amd import datatypes as dt
    from test_pair_kernels import KIND, LAYOUTS, gen, takes_b

    types = {"float_int": dt.FLOAT_INT, "double_int": dt.DOUBLE_INT, "long_int": dt.LONG_INT}
    for lname in LAYOUTS:
        a, b = gen(lname, 0, 4099), gen(lname, 1, 4099)
        td = torch.uint8 if lname in types else KIND[LAYOUTS[lname][1]]
        ta, tb = (torch.from_numpy(x.reshape(-1).copy()).view(td) for x in (a, b))
        for oname, op in (("MAXLOC", C.MAXLOC), ("MINLOC", C.MINLOC)):
            want = np.where(takes_b(lname, a, b, oname == "MAXLOC")[:, None], b, a)
            out = tb.clone()
            assert C.Reduce_local(ta, out, op, pairtype=types.get(lname)) is out  # out = ta op out
            want = np.where(takes_b(lname, a, b, oname == "MAXLOC")[:, None], b, a)
            assert np.array_equal(out.view(torch.uint8).numpy().reshape(a.shape), want), (lname, oname)
            if lname not in types:  # the op by itself: interleaved pairs, in any shape of whole pairs
                got = op(ta.view(-1, 2), tb.view(-1, 2))
                assert got.shape == (4099, 2) and np.array_equal(got.view(torch.uint8).numpy().reshape(a.shape), want)
    # a float32 view from an odd element: aligned to the member, 4 mod 8
    a, b = gen("f32x2", 0, 257), gen("f32x2", 1, 257)
    ba, bb = torch.zeros(2 * 257 + 1), torch.zeros(2 * 257 + 1)
    ba[1:].copy_(torch.from_numpy(a.reshape(-1).copy()).view(torch.float32))
    bb[1:].copy_(torch.from_numpy(b.reshape(-1).copy()).view(torch.float32))
    assert ba[1:].data_ptr() % 8 == 4
    C.Reduce_local(ba[1:], bb[1:], C.MINLOC)
    want = np.where(takes_b("f32x2", a, b, False)[:, None], b, a)
    assert np.array_equal(bb[1:].view(torch.uint8).numpy().reshape(a.shape), want) and bb[0] == 0
    assert np.array_equal(ba[1:].view(torch.uint8).numpy().reshape(a.shape), a)
    assert C.MAXLOC.Is_commutative() and C._PR_OP_CODE[C.MAXLOC] == 12 and C._PR_OP_CODE[C.MINLOC] == 13


def test_pairtype_is_checked_on_a_communicator_of_one():
    from mpit_amd import comm as C
    from mpit_amd import datatypes as dt

    W = C.Comm([0], 4243)  # (a communicator of this process alone: nothing in here communicates)
    x = torch.arange(8, dtype=torch.float32)
    y = torch.zeros(8)
    assert W.Allreduce(x, y, C.MAXLOC, algo="window") is y and torch.equal(x, y)
    raw = torch.arange(32, dtype=torch.uint8)
    out = torch.zeros(32, dtype=torch.uint8)
    W.Scan(raw, out, C.MINLOC, pairtype=dt.DOUBLE_INT)
    assert torch.equal(raw, out)
    for bad in (lambda: W.Allreduce(x[:7], y[:7], C.MAXLOC), lambda: W.Allreduce(x, y, C.SUM, pairtype=dt.FLOAT_INT),
                lambda: W.Reduce_scatter(x, y, [3], C.MINLOC),
                lambda: W.Scan(raw[1:17], out[1:17], C.MAXLOC, pairtype=dt.LONG_INT)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError, match="MPI_SHORT_INT"):
        W.Allreduce(x, y, C.MAXLOC, pairtype=dt.SHORT_INT)
    with pytest.raises(TypeError, match="MPI_LONG_DOUBLE_INT"):
        W.Reduce(x, y, C.MAXLOC, 0, pairtype=dt.LONG_DOUBLE_INT)


# ------------------------------------------------------------------ CPU tier (host shm windows)
def test_pair_reductions_cpu_three_ranks():
    _cases(run_ranks("pair_reductions.py", 3, CPU, timeout=300), ALL)


def test_pair_reductions_cpu_four_ranks():
    _cases(run_ranks("pair_reductions.py", 4, CPU, timeout=300), ALL)


# ------------------------------------------------------------------ GPU tier (ranks share the device)
@pytest.mark.gpu
def test_pair_reductions_gpu_two_ranks():
    _cases(run_ranks("pair_reductions.py", 2, GPU, timeout=300), ALL)


@pytest.mark.gpu
def test_pair_reductions_gpu_three_ranks():
    _cases(run_ranks("pair_reductions.py", 3, GPU, timeout=300), ALL)
