"""MAXLOC / MINLOC in the four reducing kernels (peer_reduce, peer_fold, peer_scan,
type_accumulate) through their raw bindings, one process: the host twins (dev = -1) on the CPU
tier, the gfx950 kernels on the GPU tier. Every comparison is bitwise, on whole pairs, against a
numpy left fold of the rule written out in its three steps:

  1. both values NaN: the pair with the smaller index; equal indices or a NaN index: the left one
  2. exactly one value NaN: that pair
  3. otherwise the better value; equal values (-0 == +0): the smaller index; equal indices or a
     NaN index: the left one

All seven interleaved layouts and the three struct layouts, sources at differing member offsets
(so an 8-byte pair sits at 4 mod 8, a 16-byte pair at 8 mod 16), guards around every
destination, sources unchanged."""
import functools

import numpy as np
import pytest
import torch

from mpit_amd import datatypes as dt
from mpit_amd._ext import native

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
MAXLOC, MINLOC = 12, 13
OPS = {"MAXLOC": MAXLOC, "MINLOC": MINLOC}
KIND = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64,
        "i32": torch.int32, "i64": torch.int64, "u8": torch.uint8}
FLOATS = ("f32", "bf16", "f16", "f64")
# name: (dtype code, value kind, index kind, index offset, extent, alignment)
LAYOUTS = {
    "f32x2": (16, "f32", "f32", 4, 8, 4), "bf16x2": (17, "bf16", "bf16", 2, 4, 2), "f16x2": (18, "f16", "f16", 2, 4, 2),
    "f64x2": (19, "f64", "f64", 8, 16, 8), "i32x2": (20, "i32", "i32", 4, 8, 4), "i64x2": (21, "i64", "i64", 8, 16, 8),
    "u8x2": (22, "u8", "u8", 1, 2, 1),
    "float_int": (24, "f32", "i32", 4, 8, 4), "double_int": (25, "f64", "i32", 8, 16, 8),
    "long_int": (26, "i64", "i32", 8, 16, 8),
}
COUNTS = [1, 2, 3, 1031, 32771]
NMAX = max(COUNTS)
NS = [1, 2, 3, 5, 8]
SRC_OFFS = [0, 1, 2, 3, 5, 7, 9, 11]  # member offset of source k: source 1 of an 8-byte pair sits at 4 mod 8
G = 32  # guard bytes on both sides of every destination
SENT = 0xA5


def dev_of(device):
    if device == "cpu":
        return -1, 0
    return torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream


def done(device):
    if device != "cpu":
        torch.cuda.synchronize()


def enc(kind, x):
    """float64 / int64 numpy values -> [n, size] bytes of the member type (exact: small values)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(KIND[kind])
    return t.view(torch.uint8).reshape(len(x), -1).numpy().copy()


def dec(kind, raw):
    """[n, size] member bytes -> float64 (floats; exact) or int64 values."""
    t = torch.from_numpy(np.ascontiguousarray(raw)).view(KIND[kind]).reshape(-1)
    return t.to(torch.float64 if kind in FLOATS else torch.int64).numpy()


def gen(lname, k, n):
    """n pairs of source k as [n, extent] bytes. Values from a handful of small numbers (ties are
    the common case), with -0 / +0, +-inf and NaN (a payload that names the source) among the
    floats; indices 0..5, so they repeat within and across sources, NaN now and then where the
    index is a float; the padding of the 16-byte struct pairs differs in every pair."""
    _, vk, ik, ioff, ext, _ = LAYOUTS[lname]
    rng = np.random.default_rng(100 * k + 7 + list(LAYOUTS).index(lname))
    if vk in FLOATS:
        v = rng.choice(np.array([0.0, -0.0, 1.0, 2.0, -1.0, 3.0, np.inf, -np.inf, np.nan]), n,
                       p=[.14, .14, .16, .16, .1, .1, .04, .04, .12])
    elif vk == "u8":
        v = rng.integers(0, 4, n)
    else:
        v = rng.integers(-2, 4, n)
    if ik in FLOATS:
        i = rng.choice(np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, np.nan]), n, p=[.16, .16, .16, .16, .16, .16, .04])
    else:
        i = rng.integers(0, 6, n)
    raw = rng.integers(0, 256, (n, ext)).astype(np.uint8)  # padding bytes: whatever is left of this
    vb, ib = enc(vk, v), enc(ik, i)
    if vk in FLOATS:
        vb[np.isnan(v), 0] |= k + 1  # low mantissa bits: the NaN's payload names its source
    if ik in FLOATS:
        ib[np.isnan(i), 0] |= k + 1
    raw[:, : vb.shape[1]] = vb
    raw[:, ioff: ioff + ib.shape[1]] = ib
    return raw


def takes_b(lname, a, b, maximum):
    """The rule, step by step, on [n, extent] byte arrays: True where (a, b) gives b."""
    _, vk, ik, ioff, _, _ = LAYOUTS[lname]
    vs, isz = KIND[vk].itemsize, KIND[ik].itemsize
    va, vb = dec(vk, a[:, :vs]), dec(vk, b[:, :vs])
    ia, ib = dec(ik, a[:, ioff: ioff + isz]), dec(ik, b[:, ioff: ioff + isz])
    an = np.isnan(va) if vk in FLOATS else np.zeros(len(va), bool)
    bn = np.isnan(vb) if vk in FLOATS else np.zeros(len(vb), bool)
    with np.errstate(invalid="ignore"):
        smaller_idx = ib < ia  # False when either is NaN
        b_better = (vb > va) if maximum else (vb < va)
        a_better = (va > vb) if maximum else (va < vb)
    out = np.zeros(len(va), bool)
    both, one, none = an & bn, an ^ bn, ~an & ~bn
    out[both] = smaller_idx[both]                                         # 1.
    out[one] = bn[one]                                                    # 2.
    out[none] = (b_better | (~a_better & smaller_idx))[none]              # 3.
    return out


@functools.lru_cache(maxsize=None)
def sources(lname):
    return tuple(gen(lname, k, NMAX) for k in range(8))


@functools.lru_cache(maxsize=None)
def prefixes(lname, oname):
    """prefix[j] = ((s0 op s1) op ...) op sj as [NMAX, extent] bytes; computed once."""
    out, acc = [], None
    for s in sources(lname):
        acc = s if acc is None else np.where(takes_b(lname, acc, s, oname == "MAXLOC")[:, None], s, acc)
        out.append(acc)
    return tuple(out)


SLOT = 64  # byte offset of member offset 0 inside a source buffer (a multiple of 16)


@functools.lru_cache(maxsize=None)
def on_device(lname, device):
    """Eight buffers; source k starts SLOT + SRC_OFFS[k] * alignment bytes into buffer k."""
    ext, al = LAYOUTS[lname][4], LAYOUTS[lname][5]
    bufs = []
    for k, s in enumerate(sources(lname)):
        h = np.full(SLOT + max(SRC_OFFS) * al + NMAX * ext + SLOT, SENT, np.uint8)
        at = SLOT + SRC_OFFS[k] * al
        h[at: at + NMAX * ext] = s.reshape(-1)
        bufs.append(torch.from_numpy(h).to(device))
        assert bufs[-1].data_ptr() % 16 == 0
    return tuple(bufs)


def host_copy(lname, k):
    ext, al = LAYOUTS[lname][4], LAYOUTS[lname][5]
    h = np.full(SLOT + max(SRC_OFFS) * al + NMAX * ext + SLOT, SENT, np.uint8)
    at = SLOT + SRC_OFFS[k] * al
    h[at: at + NMAX * ext] = sources(lname)[k].reshape(-1)
    return h


def src_ptrs(lname, bufs, ns):
    al = LAYOUTS[lname][5]
    return [bufs[k].data_ptr() + SLOT + SRC_OFFS[k] * al for k in range(ns)]


def guarded(device, lname, cnt, doff):
    """(device buffer, byte position of the destination, host image) of a destination `doff`
    members past a 16-byte boundary, sentinel guards around it."""
    ext, al = LAYOUTS[lname][4], LAYOUTS[lname][5]
    h = np.full(G + doff * al + cnt * ext + G, SENT, np.uint8)
    t = torch.from_numpy(h.copy()).to(device)
    assert t.data_ptr() % 16 == 0
    return t, G + doff * al, h


def expect(h, at, rows):
    w = h.copy()
    w[at: at + rows.size] = rows.reshape(-1)
    return w


def same(t, want, tag):
    got = t.cpu().numpy()
    assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:8])


def unchanged(lname, device):
    for k, b in enumerate(on_device(lname, device)):
        assert np.array_equal(b.cpu().numpy(), host_copy(lname, k)), "source modified"


CASES = [(ln, on) for ln in LAYOUTS for on in OPS]


def test_the_data_holds_the_cases_the_rule_names():
    """Ties, -0 against +0, NaN on one side and on both at equal and at different indices, NaN
    indices, and destinations that sit off the pair's own alignment."""
    a, b = sources("f32x2")[0], sources("f32x2")[1]
    va, vb, ia, ib = dec("f32", a[:, :4]), dec("f32", b[:, :4]), dec("f32", a[:, 4:]), dec("f32", b[:, 4:])
    assert ((va == vb) & (ia == ib)).any() and ((va == vb) & (ia != ib)).any()
    assert ((va == 0) & (vb == 0) & (np.signbit(va) != np.signbit(vb))).any()
    assert (np.isnan(va) & np.isnan(vb) & (ia == ib)).any() and (np.isnan(va) & np.isnan(vb) & (ia != ib)).any()
    assert (np.isnan(va) ^ np.isnan(vb)).any() and (np.isinf(va) & np.isinf(vb)).any()
    assert ((va == vb) & np.isnan(ia)).any() and ((va == vb) & np.isnan(ib)).any()
    assert (SLOT + SRC_OFFS[1] * 4) % 8 == 4 and (G + 1 * 4) % 8 == 4  # source 1 and doff 1: 4 mod 8
    pad = sources("double_int")[0][:, 12:]
    assert len(np.unique(pad.view(np.uint32))) > 1000  # the padding differs from pair to pair
    # the two orders of one non-degenerate pair of operands disagree only through the rule's ties
    assert takes_b("f32x2", a, b, True).any() and not takes_b("f32x2", a, a, True).any()


# ------------------------------------------------------------------ peer_reduce and peer_fold
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("lname,oname", CASES)
def test_peer_reduce_and_fold(device, lname, oname):
    """Counts x ns x destination member offsets {0, 1, 3}: peer_reduce into two destinations at
    different offsets (the second always one member off the first) and peer_fold with max_blocks
    1 and 3 (the grid-stride loop) give the oracle's bytes and leave the guards alone."""
    dcode, ext = LAYOUTS[lname][0], LAYOUTS[lname][4]
    nat, (dev, stream) = native(), dev_of(device)
    bufs = on_device(lname, device)
    pre = prefixes(lname, oname)
    for cnt in COUNTS:
        for ns in NS:
            rows = pre[ns - 1][:cnt]
            for doff in (0, 1, 3):
                tag = (lname, oname, cnt, ns, doff)
                d0, at0, h0 = guarded(device, lname, cnt, doff)
                d1, at1, h1 = guarded(device, lname, cnt, doff + 1)
                nat.peer_reduce(dev, stream, OPS[oname], dcode, src_ptrs(lname, bufs, ns),
                                [d0.data_ptr() + at0, d1.data_ptr() + at1], cnt)
                done(device)
                same(d0, expect(h0, at0, rows), (tag, "peer_reduce dst 0"))
                same(d1, expect(h1, at1, rows), (tag, "peer_reduce dst 1"))
                for mb in (1, 3):
                    f, at, h = guarded(device, lname, cnt, doff)
                    nat.peer_fold(dev, stream, OPS[oname], dcode, src_ptrs(lname, bufs, ns), f.data_ptr() + at, cnt, mb)
                    done(device)
                    same(f, expect(h, at, rows), (tag, mb, "peer_fold"))
                    assert torch.equal(f.cpu(), d0.cpu()), (tag, mb, "peer_fold differs from peer_reduce")
    unchanged(lname, device)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("lname", list(LAYOUTS))
def test_peer_reduce_in_place(device, lname):
    """dst[j] = src[j] for every j, each at its own member offset: what the window all-reduce runs."""
    dcode, ext, al = LAYOUTS[lname][0], LAYOUTS[lname][4], LAYOUTS[lname][5]
    nat, (dev, stream) = native(), dev_of(device)
    for cnt, ns in ((1031, 3), (32771, 8), (3, 2)):
        work = [b.clone() for b in on_device(lname, device)[:ns]]
        ptrs = src_ptrs(lname, work, ns)
        nat.peer_reduce(dev, stream, MAXLOC, dcode, ptrs, ptrs, cnt)
        done(device)
        for j in range(ns):
            at = SLOT + SRC_OFFS[j] * al
            same(work[j], expect(host_copy(lname, j), at, prefixes(lname, "MAXLOC")[ns - 1][:cnt]), (lname, cnt, ns, j))


# ------------------------------------------------------------------ peer_scan
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("lname,oname", CASES)
def test_peer_scan(device, lname, oname):
    """Inclusive and exclusive, in place and out of place: prefix j is the fold of sources 0..j
    (0..j-1 exclusive; dst[0] untouched then), and the last one is peer_reduce's result."""
    dcode, ext, al = LAYOUTS[lname][0], LAYOUTS[lname][4], LAYOUTS[lname][5]
    nat, (dev, stream) = native(), dev_of(device)
    bufs = on_device(lname, device)
    pre = prefixes(lname, oname)
    for cnt in COUNTS:
        for ns in NS:
            for excl in (False, True):
                for inplace in (False, True):
                    for mb in ((1, 3) if cnt == NMAX or ns == 8 else (0,)):
                        tag = (lname, oname, cnt, ns, excl, inplace, mb)
                        if inplace:
                            work = [b.clone() for b in bufs[:ns]]
                            ptrs = src_ptrs(lname, work, ns)
                            nat.peer_scan(dev, stream, OPS[oname], dcode, excl, ptrs, ptrs, cnt, mb)
                            done(device)
                            for j in range(ns):
                                want = host_copy(lname, j)
                                if not (excl and j == 0):
                                    want = expect(want, SLOT + SRC_OFFS[j] * al, pre[j - 1 if excl else j][:cnt])
                                same(work[j], want, (tag, j))
                            lo = SLOT + SRC_OFFS[ns - 1] * al
                            last = work[ns - 1][lo: lo + cnt * ext]
                        else:
                            outs = [guarded(device, lname, cnt, (3 * j + 1) % 5) for j in range(ns)]
                            nat.peer_scan(dev, stream, OPS[oname], dcode, excl, src_ptrs(lname, bufs, ns),
                                          [o[0].data_ptr() + o[1] for o in outs], cnt, mb)
                            done(device)
                            for j, (t, at, h) in enumerate(outs):
                                want = h if excl and j == 0 else expect(h, at, pre[j - 1 if excl else j][:cnt])
                                same(t, want, (tag, j))
                            t, at, _ = outs[ns - 1]
                            last = t[at: at + cnt * ext]
                        nred = ns - 1 if excl else ns
                        if nred >= 1:
                            red = torch.zeros(cnt * ext, dtype=torch.uint8).to(device)
                            nat.peer_reduce(dev, stream, OPS[oname], dcode, src_ptrs(lname, bufs, nred),
                                            [red.data_ptr()], cnt)
                            done(device)
                            assert torch.equal(last.cpu(), red.cpu()), (tag, "peer_reduce differs")
    unchanged(lname, device)


# ------------------------------------------------------------------ type_accumulate
def acc_case(device, lname, oname, vector, fetch, soff=0, raises=None):
    """target = op(target, origin) pair by pair on a contiguous run of 1031 pairs or on two
    instances of a vector of five 3-pair blocks every 7 pairs; target = source 0, origin = source 1."""
    dcode, ext = LAYOUTS[lname][0], LAYOUTS[lname][4]
    if vector:
        t, count = dt.Type_vector(5, 3 * ext, 7 * ext, dt.BYTE), 2
        span = (4 * 7 + 3) * ext
        first = np.concatenate([np.arange(3 * ext) + b * 7 * ext for b in range(5)])
        idx = np.concatenate([first + c * span for c in range(count)])
    else:
        t, count = dt.Type_contiguous(1031 * ext, dt.BYTE), 1
        idx = np.arange(1031 * ext)
    npair = len(idx) // ext
    tv, ov = sources(lname)[0][:npair], sources(lname)[1][:npair]
    tbuf = np.full(G + soff + int(idx.max()) + 1 + G, SENT, np.uint8)
    tbuf[G + soff + idx] = tv.reshape(-1)
    obuf = np.full(G + npair * ext + G, SENT, np.uint8)
    obuf[G: G + npair * ext] = ov.reshape(-1)
    fbuf = np.full(G + npair * ext + G, SENT, np.uint8)
    T, O, F = (torch.from_numpy(x.copy()).to(device) for x in (tbuf, obuf, fbuf))
    plan = t.plan(count)
    tab, off, _keep = plan.table(T.device)
    sp, pp = T.data_ptr() + G + soff + off, O.data_ptr() + G
    fp = F.data_ptr() + G if fetch else 0
    unit = plan.unit(sp, pp | fp)
    dev, stream = dev_of(device)
    args = (dev, stream, OPS[oname], dcode, sp, pp, fp, plan._loops, tab, plan.R, plan.L, plan.per, unit)
    tag = (lname, oname, vector, fetch, soff, unit)
    if raises is not None:
        assert unit < ext, tag
        with pytest.raises(raises) as ei:
            native().type_accumulate(*args)
        assert str(ext) in str(ei.value) and str(unit) in str(ei.value), ei.value  # names the pair and the unit
        want_t, want_f = tbuf, fbuf
    else:
        assert unit >= ext, tag
        native().type_accumulate(*args)
        done(device)
        res = np.where(takes_b(lname, tv, ov, oname == "MAXLOC")[:, None], ov, tv)
        want_t = tbuf.copy()
        want_t[G + soff + idx] = res.reshape(-1)
        want_f = expect(fbuf, G, tv) if fetch else fbuf  # the fetch is the target's previous bytes
    same(T, want_t, (tag, "target"))
    same(O, obuf, (tag, "origin"))
    same(F, want_f, (tag, "fetch"))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("lname,oname", CASES)
def test_type_accumulate_pairs(device, lname, oname):
    for vector in (False, True):
        for fetch in (False, True):
            acc_case(device, lname, oname, vector, fetch)
    ext, al = LAYOUTS[lname][4], LAYOUTS[lname][5]
    if ext > al:  # a target aligned to its largest member only: the item is smaller than the pair
        acc_case(device, lname, oname, False, True, soff=al, raises=ValueError)


# ------------------------------------------------------------------ the support matrix
def test_support_matrix():
    """The pair ops on the pair layouts and nowhere else, every other op refused on them, REPLACE
    / NO_OP too; the old (op, dtype) answers as they were, their codes included."""
    nat = native()
    pair_codes = [v[0] for v in LAYOUTS.values()]
    assert (nat.PR_MAXLOC, nat.PR_MINLOC, nat.ACC_REPLACE, nat.ACC_NO_OP) == (12, 13, 10, 11)
    assert (nat.PR_PAIR, nat.PR_FLOAT_INT, nat.PR_DOUBLE_INT, nat.PR_LONG_INT) == (16, 24, 25, 26)
    for d in range(-1, 40):
        for op in range(-1, 20):
            pr, acc = nat.peer_reduce_supported(op, d), nat.type_accumulate_supported(op, d)
            if d in pair_codes:
                assert pr == acc == (op in (MAXLOC, MINLOC)), (op, d)
            elif 0 <= d < 7:
                integer = d in (4, 5, 6)
                assert pr == (0 <= op < 7 or (7 <= op < 10 and integer)), (op, d)
                assert acc == (pr or op in (10, 11)), (op, d)
            else:
                assert not pr and not acc, (op, d)
    for name, (code, _, _, _, ext, al) in LAYOUTS.items():
        assert nat.peer_dtype_size(code) == ext and nat.peer_dtype_align(code) == al, name
    x = torch.zeros(64, dtype=torch.uint8)
    for fn in (lambda op, d, p: nat.peer_reduce(-1, 0, op, d, [p], [p + 32], 2),
               lambda op, d, p: nat.peer_fold(-1, 0, op, d, [p], p + 32, 2, 0),
               lambda op, d, p: nat.peer_scan(-1, 0, op, d, False, [p], [p + 32], 2, 0)):
        with pytest.raises(ValueError):
            fn(0, 16, x.data_ptr())  # SUM on pairs
        with pytest.raises(ValueError):
            fn(MAXLOC, 0, x.data_ptr())  # MAXLOC on scalars
        with pytest.raises(ValueError):
            fn(MAXLOC, 16, x.data_ptr() + 2)  # a float32 pair off its member's alignment
        fn(MAXLOC, 16, x.data_ptr() + 4)  # ... and on it
