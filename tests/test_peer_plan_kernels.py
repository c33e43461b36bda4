"""peer_plan_gather (csrc/kernels/peer_plan.hip): up to 8 layout-to-layout copies in one launch,
through the raw binding; the host twin in the CPU tier, the kernel under -m gpu on the same cases.

Both sides of a segment are `count` instances of a Datatype: the kernel gets the type's Plan
(loops, run table), the oracle is the type's byte index (Datatype._byte_index, the index path that
never builds a plan), so dst[didx[q]] = src[sidx[q]] for every packed byte q. Every comparison is
bitwise and over the whole destination arena: the segments' regions lie between sentinel bytes,
so a stray store anywhere fails. The tile is 1,024 items of `unit` bytes."""
import numpy as np
import pytest
import torch

from mpit_amd import datatypes as dt
from mpit_amd._ext import native

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
G, SENT = 64, 0xA5
LDS_RUNS = 1024  # tl::kLdsRuns: run tables up to this length are staged in LDS


def low_bit(x):
    return 16 if x % 16 == 0 else (x & -x)


def side(t, count, buf, at, device):
    """(base address, layout tuple, byte index relative to buf, plan, keep-alive) of `count` x t
    whose origin is byte `at` of buf."""
    plan = t.plan(count)
    idx = t._byte_index(count, "cpu").numpy() + at
    if plan.total == 0:
        return buf.data_ptr() + at, None, idx, plan, None
    tab, off, keep = plan.table(torch.device(device) if device == "cpu" else buf.device)
    return buf.data_ptr() + at + off, (list(plan.loops), tab, plan.R, plan.L, plan.per), idx, plan, keep


def empty_layout(unit):
    return ([(0, 0)], 0, 1, unit, unit)


def span(t, count):
    p = t.plan(count)
    return p.hi if p.total else 0


def run(device, specs, max_blocks=0, wide=False, units=None, expect_units=None):
    """specs: [(src type, src count, src byte offset mod 16, dst type, dst count, dst offset mod 16)].
    Each side gets its own 16-byte aligned region of one source and one destination arena."""
    nat = native()
    dev = -1 if device == "cpu" else torch.cuda.current_device()
    stream = 0 if device == "cpu" else torch.cuda.current_stream().cuda_stream
    s_at, d_at, sp, dp = [], [], G, G
    for st, sc, so, dty, dc, do in specs:
        s_at.append(sp + so)
        d_at.append(dp + do)
        sp += (so + span(st, sc) + G + 15) & ~15
        dp += (do + span(dty, dc) + G + 15) & ~15
    host = np.random.default_rng(len(specs) * 7 + sp).integers(1, 256, sp, dtype=np.uint8)  # never a sentinel run
    src = torch.from_numpy(host).to(device)
    dst = torch.full((dp,), SENT, dtype=torch.uint8, device=device)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    exp = np.full(dp, SENT, dtype=np.uint8)
    segs, keep, got_units = [], [], []
    for k, (st, sc, so, dty, dc, do) in enumerate(specs):
        sb, sl, sidx, splan, k1 = side(st, sc, src, s_at[k], device)
        db, dl, didx, dplan, k2 = side(dty, dc, dst, d_at[k], device)
        keep += [k1, k2]
        assert len(sidx) == len(didx)
        exp[didx] = host[sidx]
        unit = low_bit(splan.align | dplan.align | sb | db) if units is None else units[k]
        got_units.append(unit)
        segs.append((sb, sl or empty_layout(unit), db, dl or empty_layout(unit), unit))
    if expect_units is not None:
        assert got_units == expect_units, got_units
    nat.peer_plan_gather(dev, stream, segs, max_blocks, wide)
    assert np.array_equal(dst.cpu().numpy(), exp), (specs, max_blocks, wide)
    assert np.array_equal(src.cpu().numpy(), host), "a source was modified"
    return got_units


def contiguous(nbytes):
    return dt.Type_contiguous(nbytes, dt.BYTE)


def nest(depth, b, pad):
    """24 * b bytes in blocks of b under `depth` loops (0: contiguous); strides multiples of pad."""
    if depth == 0:
        return contiguous(24 * b), 1
    if depth == 1:
        return dt.Type_create_hvector(24, b, b + pad, dt.BYTE), 1
    if depth == 2:
        inner = dt.Type_create_hvector(6, b, b + pad, dt.BYTE)
        return dt.Type_create_hvector(4, 1, 6 * (b + pad) + 3 * pad, inner), 1
    inner = dt.Type_create_hvector(4, b, b + pad, dt.BYTE)
    mid = dt.Type_create_hvector(3, 1, 4 * (b + pad) + pad, inner)
    return dt.Type_create_resized(mid, 0, 3 * (4 * (b + pad) + pad) + 5 * pad), 2


def runs_type(mode, step, seed=0):
    """48 * step bytes per instance in run mode 0 (one run), 1 (equal runs) or 2 (unequal runs)."""
    if mode == 0:
        return contiguous(48 * step)
    lens = np.array([8] * 6 if mode == 1 else [4, 12, 8, 16, 2, 6]) * step
    gaps = np.roll([1, 2, 4, 1, 3, 2], seed) * step  # (never a progression: the table stays whole)
    offs = np.concatenate([[0], np.cumsum(lens + gaps)[:-1]])
    return dt.Type_create_hindexed([int(x) for x in lens], [int(x) for x in offs], dt.BYTE)


def long_table(R, equal, seed, gap_seed=0):
    """R runs (equal: 8 bytes each, else 1..16 from `seed`) at gaps of 1..8 bytes from `gap_seed`."""
    lens = np.full(R, 8) if equal else np.random.default_rng(seed).integers(1, 17, R)
    gaps = np.random.default_rng(1000 + gap_seed).integers(1, 9, R)
    offs = np.concatenate([[0], np.cumsum(lens + gaps)[:-1]])
    return dt.Type_create_hindexed([int(x) for x in lens], [int(x) for x in offs], dt.BYTE)


# ------------------------------------------------------------------ item counts and units
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("unit", [1, 2, 4, 8, 16])
def test_item_counts_and_units(device, unit):
    """0, 1, 1023, 1024 and 1025 items of every unit; the unit forced by the stride and run length
    (aligned addresses) and by an address (16-byte layouts)."""
    for n in (0, 1, 1023, 1024, 1025):
        by_stride = dt.Type_create_hvector(n, unit, 3 * unit, dt.BYTE)
        run(device, [(by_stride, 1, 0, contiguous(n * unit), 1, 0)], expect_units=[unit] if n else None)
        run(device, [(contiguous(n * unit), 1, 0, by_stride, 1, 0)], expect_units=[unit] if n else None)
    for n16 in (1, 64, 65):  # 16-byte blocks, 1,024 and 1,040 bytes around the tile for unit 1
        wide16 = dt.Type_create_hvector(n16, 16, 48, dt.BYTE)
        run(device, [(wide16, 1, unit % 16, contiguous(n16 * 16), 1, 0)], expect_units=[unit])
        run(device, [(wide16, 1, 0, wide16, 1, unit % 16)], expect_units=[unit])


# ------------------------------------------------------------------ loops and run modes
@pytest.mark.parametrize("device", DEVICES)
def test_zero_to_three_loops_per_side(device):
    for b, pad in ((1, 1), (4, 4), (16, 16)):
        for ds in range(4):
            for dd in range(4):
                st, sc = nest(ds, b, pad)
                dty, dc = nest(dd, b, 2 * pad)
                assert len(st.plan(sc).loops) == ds and len(dty.plan(dc).loops) == dd
                run(device, [(st, sc, 0, dty, dc, 0)], expect_units=[b] if ds + dd else None)


@pytest.mark.parametrize("device", DEVICES)
def test_all_nine_run_mode_pairs(device):
    for step in (1, 4):
        for sm in range(3):
            for dm in range(3):
                st, dty = runs_type(sm, step, seed=1), runs_type(dm, step, seed=5)
                ps, pd = st.plan(3), dty.plan(3)
                for p, m in ((ps, sm), (pd, dm)):
                    assert (p.R == 1, p.L != 0) == ((True, True), (False, True), (False, False))[m], (p, m)
                run(device, [(st, 3, 0, dty, 3, 0)])
    # 25 tiles through the two table modes at once, 1 and 3 blocks
    for mb in (1, 3):
        run(device, [(runs_type(2, 1), 533, 0, runs_type(1, 1), 533, 0)], max_blocks=mb)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("R", [LDS_RUNS - 1, LDS_RUNS + 1])
def test_tables_below_and_above_the_lds_cap(device, R):
    for equal in (True, False):
        t = long_table(R, equal, seed=R)
        p = t.plan(2)
        assert p.R == R and (p.L != 0) == equal
        run(device, [(t, 2, 0, contiguous(p.total), 1, 0)])
        run(device, [(contiguous(p.total), 1, 0, t, 2, 0)], max_blocks=2)
        run(device, [(t, 2, 0, long_table(R, equal, seed=R, gap_seed=1), 2, 0)])


# ------------------------------------------------------------------ several segments in one grid
def eight_segments():
    big = dt.Type_create_hvector(2500, 4, 12, dt.BYTE)  # 10,000 bytes: 3 tiles of unit 4
    t2 = runs_type(2, 1, seed=3)
    return [
        (contiguous(3), 1, 5, contiguous(3), 1, 9),  # 3 bytes
        (big, 1, 0, contiguous(10000), 1, 0),
        (big, 0, 0, contiguous(0), 1, 0),  # empty
        (t2, 40, 0, runs_type(1, 1, seed=4), 40, 0),  # 1,920 bytes: 2 tiles of unit 1, both tables
        (contiguous(4100), 1, 2, dt.Type_create_hvector(2050, 2, 6, dt.BYTE), 1, 0),  # unit 2, 3 tiles
        (long_table(LDS_RUNS + 1, False, 9), 1, 0, contiguous(long_table(LDS_RUNS + 1, False, 9).plan(1).total), 1, 0),
        (nest(3, 16, 16)[0], 2, 0, nest(2, 16, 32)[0], 1, 0),  # unit 16
        (contiguous(1024 * 8 + 8), 1, 8, dt.Type_create_hvector(1025, 8, 24, dt.BYTE), 1, 0),  # unit 8, 1,025 items
    ]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("max_blocks", [0, 1, 3])
def test_one_three_and_eight_segments(device, max_blocks):
    """A 3-byte segment beside a multi-tile one with an empty one between; with max_blocks 1 and 3
    one block crosses segments of different units, modes and tables."""
    segs = eight_segments()
    run(device, segs[1:2], max_blocks=max_blocks)
    units = run(device, segs[:3], max_blocks=max_blocks)
    assert units[:2] == [1, 4]
    units = run(device, segs, max_blocks=max_blocks)
    assert sorted(set(units)) == [1, 2, 4, 8, 16]
    run(device, list(reversed(segs)), max_blocks=max_blocks)


@pytest.mark.parametrize("device", DEVICES)
def test_wide_indices_on_a_small_case(device):
    run(device, eight_segments()[:5], wide=True)
    run(device, [(runs_type(2, 4), 100, 0, nest(1, 16, 16)[0], 50, 0)], max_blocks=2, wide=True)


@pytest.mark.parametrize("device", DEVICES)
def test_identical_source_and_destination_is_dropped(device):
    """A segment whose sides are the same address and layout moves nothing (an in-place part); the
    segments beside it still move."""
    nat = native()
    dev = -1 if device == "cpu" else torch.cuda.current_device()
    stream = 0 if device == "cpu" else torch.cuda.current_stream().cuda_stream
    host = np.random.default_rng(2).integers(1, 256, 4096, dtype=np.uint8)
    a = torch.from_numpy(host).to(device)
    out = torch.full((512,), SENT, dtype=torch.uint8, device=device)
    lay = ([(10, 48)], 0, 1, 16, 16)
    same = (a.data_ptr() + 64, lay, a.data_ptr() + 64, lay, 16)
    move = (a.data_ptr() + 1024, lay, out.data_ptr() + 32, ([], 0, 1, 160, 160), 16)
    nat.peer_plan_gather(dev, stream, [same, move, same], 1, False)
    assert np.array_equal(a.cpu().numpy(), host)
    exp = np.full(512, SENT, dtype=np.uint8)
    exp[32:192] = host[1024:1024 + 480].reshape(10, 48)[:, :16].reshape(-1)
    assert np.array_equal(out.cpu().numpy(), exp)
    nat.peer_plan_gather(dev, stream, [same], 0, False)  # nothing left: no launch
    nat.peer_plan_gather(dev, stream, [], 0, False)


# ------------------------------------------------------------------ refusals
def test_refusals_before_any_launch():
    nat = native()
    x = torch.full((256,), 1, dtype=torch.uint8)
    y = torch.full((256,), SENT, dtype=torch.uint8)
    vec, flat = ([(4, 32)], 0, 1, 8, 8), ([], 0, 1, 32, 32)
    ok = (x.data_ptr(), vec, y.data_ptr(), flat, 8)
    nat.peer_plan_gather(-1, 0, [ok] * 1)
    y.fill_(SENT)
    bad_cases = [
        [(x.data_ptr(), vec, y.data_ptr(), ([], 0, 1, 24, 24), 8)],  # unequal packed sizes
        [(x.data_ptr(), ([(5, 32)], 0, 1, 8, 8), y.data_ptr(), flat, 8)],
        [ok] * 9,  # nine segments
        [(x.data_ptr(), vec, y.data_ptr(), flat, 16)],  # a unit that divides neither the run nor ...
        [(x.data_ptr(), ([(4, 36)], 0, 1, 8, 8), y.data_ptr(), flat, 8)],  # ... a stride
        [(x.data_ptr() + 4, vec, y.data_ptr(), flat, 8)],  # ... the source address
        [(x.data_ptr(), vec, y.data_ptr() + 2, flat, 8)],  # ... the destination address
        [(x.data_ptr(), vec, y.data_ptr(), flat, 3)],
        [(x.data_ptr(), vec, y.data_ptr(), ([(1, 0)] * 4, 0, 1, 32, 32), 8)],  # four loops
        [ok, (x.data_ptr(), vec, y.data_ptr() + 64, ([], 0, 1, 16, 16), 8)],  # a bad one behind a good one
    ]
    for segs in bad_cases:
        with pytest.raises(ValueError):
            nat.peer_plan_gather(-1, 0, segs)
        assert bool((y == SENT).all()), "bytes moved before the refusal"
