"""The kernels of the window collectives (csrc/kernels/peer_coll.hip) through their raw bindings,
one process: peer_gather, peer_fold and peer_scan, and peer_reduce's vector body (every pointer
at one offset within 16 bytes), the host twins (dev = -1) on the CPU tier and the gfx950 kernels
on the GPU tier. Every comparison is bitwise: against the source bytes
(peer_gather), against the left fold in the order given computed with torch on the CPU (16-bit
floats folded in fp32 and cast once) and against peer_reduce on the same operands (peer_fold,
peer_scan). Guards around every destination and the sources themselves must stay as they were."""
import functools

import pytest
import torch

from mpit_amd import comm as C
from mpit_amd._ext import native

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
G = 32  # guard elements (bytes for peer_gather) on both sides of every destination
COUNTS = [1, 3, 1031, 65541]
NMAX = max(COUNTS)
SRC_OFFS = [0, 1, 2, 3, 5, 7, 9, 11]  # element offset of source k: their 16-byte alignments differ
NS = [1, 2, 3, 5, 8]
FLOATS = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
INTS = [torch.int32, torch.int64, torch.uint8]
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
OPS = {"SUM": C.SUM, "PROD": C.PROD, "MAX": C.MAX, "MIN": C.MIN, "LAND": C.LAND, "LOR": C.LOR, "LXOR": C.LXOR,
       "BAND": C.BAND, "BOR": C.BOR, "BXOR": C.BXOR}
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64, "i32": torch.int32,
      "i64": torch.int64, "u8": torch.uint8}
PAIRS = [("SUM", "f32"), ("SUM", "bf16"), ("SUM", "f16"), ("PROD", "f64"), ("MAX", "i64"), ("BXOR", "u8"),
         ("LXOR", "i32")]
OTHER_PAIRS = [(o, d) for d, t in DT.items() for o in OPS
               if (o, d) not in PAIRS and (t in INTS or o not in ("BAND", "BOR", "BXOR"))]


def dev_of(device):
    if device == "cpu":
        return -1, 0
    return torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream


def done(device):
    if device != "cpu":
        torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def same(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a.cpu()), bits(b.cpu())))


def gen(dtype, k, length):
    """Source k: floats span about 2^+-20 in magnitude (2^+-4 for fp16) so that the order of
    addition shows in the bits; a quarter of the elements are +0 (the logical ops need both)."""
    g = torch.Generator().manual_seed(1000 * k + 11 + (FLOATS + INTS).index(dtype))
    if dtype in FLOATS:
        e = 4 if dtype == torch.float16 else 20
        x = torch.randn(length, generator=g, dtype=torch.float64) * \
            torch.pow(2.0, torch.randint(-e, e + 1, (length,), generator=g).double())
        x[torch.rand(length, generator=g) < 0.25] = 0.0
        return x.to(dtype)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (length,), generator=g, dtype=torch.int64).to(torch.uint8)
    return torch.randint(-50, 51, (length,), generator=g, dtype=torch.int64).to(dtype)


@functools.lru_cache(maxsize=None)
def sources(dname):
    """Eight host buffers; source k is buf[k][SRC_OFFS[k]: SRC_OFFS[k] + NMAX]."""
    return tuple(gen(DT[dname], k, max(SRC_OFFS) + NMAX + 4) for k in range(8))


@functools.lru_cache(maxsize=None)
def prefixes(oname, dname):
    """prefix[j] = ((s0 op s1) op ...) op sj over NMAX elements, wide, cast once; computed once."""
    dt, op = DT[dname], OPS[oname]
    wide = torch.float32 if dt in (torch.bfloat16, torch.float16) else dt
    out, acc = [], None
    for k, b in enumerate(sources(dname)):
        x = b[SRC_OFFS[k]: SRC_OFFS[k] + NMAX].to(wide)
        acc = x if acc is None else op(acc, x)
        out.append(acc.to(dt))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def on_device(dname, device):
    return tuple(b.clone().to(device) for b in sources(dname))


def src_ptrs(bufs, ns):
    es = bufs[0].element_size()
    return [bufs[k].data_ptr() + SRC_OFFS[k] * es for k in range(ns)]


# ------------------------------------------------------------------ peer_gather
GLENS = [0, 1, 15, 16, 17, 4099, 262164, 33]
SMIS = [0, 1, 3, 8]
DMIS = [0, 2, 5, 12]


def gather_case(device, lens, smis, dmis, max_blocks):
    """Segment g: lens[g] bytes from a 16-byte-aligned slot + smis[g] to a slot + dmis[g]."""
    gsrc = torch.Generator().manual_seed(5)
    spos, dpos, s_at, d_at = [], [], 16, G
    for ln, sm, dm in zip(lens, smis, dmis):
        spos.append(s_at + sm)
        dpos.append(d_at + dm)
        s_at += (ln + sm + 15) // 16 * 16 + 16
        d_at += (ln + dm + 15) // 16 * 16 + 2 * G
    src_h = torch.randint(0, 256, (s_at,), generator=gsrc, dtype=torch.int64).to(torch.uint8)
    dst_h = torch.full((d_at,), 0xA5, dtype=torch.uint8)
    want = dst_h.clone()
    for ln, sp, dp in zip(lens, spos, dpos):
        want[dp: dp + ln] = src_h[sp: sp + ln]
    src, dst = src_h.clone().to(device), dst_h.clone().to(device)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    dev, stream = dev_of(device)
    native().peer_gather(dev, stream, [src.data_ptr() + p for p in spos], [dst.data_ptr() + p for p in dpos],
                         list(lens), max_blocks)
    done(device)
    assert torch.equal(dst.cpu(), want), (lens, smis, dmis, max_blocks)
    assert torch.equal(src.cpu(), src_h), "source modified"


@pytest.mark.parametrize("device", DEVICES)
def test_peer_gather_eight_segments_every_misalignment(device):
    """Lengths {0, 1, 15, 16, 17, 4099, 262164} (and 33) mixed in one call; every source
    misalignment {0, 1, 3, 8} x destination misalignment {0, 2, 5, 12} on every segment;
    max_blocks 1 and 3 (the grid-stride loop) and 0."""
    for i in range(4):
        for j in range(4):
            sm = [SMIS[(i + g) % 4] for g in range(8)]
            dm = [DMIS[(j + g) % 4] for g in range(8)]
            for mb in (1, 3, 0):
                gather_case(device, GLENS, sm, dm, mb)
    gather_case(device, GLENS[::-1], [SMIS[g % 4] for g in range(8)], [DMIS[(g + 1) % 4] for g in range(8)], 3)


@pytest.mark.parametrize("device", DEVICES)
def test_peer_gather_one_segment_and_dropped_segments(device):
    for ln in GLENS:
        for i in range(4):
            for mb in (1, 0):
                gather_case(device, [ln], [SMIS[i]], [DMIS[(i + 1) % 4]], mb)
    # src == dst is dropped, nothing but zero-length segments launches nothing, nine are refused
    dev, stream = dev_of(device)
    t = torch.arange(64, dtype=torch.uint8).to(device)
    native().peer_gather(dev, stream, [t.data_ptr(), t.data_ptr() + 3], [t.data_ptr(), t.data_ptr() + 40], [64, 0], 0)
    native().peer_gather(dev, stream, [], [], [], 0)
    done(device)
    assert torch.equal(t.cpu(), torch.arange(64, dtype=torch.uint8))
    with pytest.raises(Exception):
        native().peer_gather(dev, stream, [t.data_ptr()] * 9, [t.data_ptr() + 1] * 9, [1] * 9, 0)


# ------------------------------------------------------------------ peer_fold
def fold_case(device, oname, dname, cnt, doff, ns, max_blocks):
    dt = DT[dname]
    code, dcode = C._PR_OP_CODE[OPS[oname]], C._PR_DTYPES[dt]
    bufs = on_device(dname, device)
    es = bufs[0].element_size()
    guard = gen(dt, 77, G + 3 + NMAX + G)[: G + doff + cnt + G]
    out, ref = guard.clone().to(device), guard.clone().to(device)
    want = guard.clone()
    want[G + doff: G + doff + cnt] = prefixes(oname, dname)[ns - 1][:cnt]
    dev, stream = dev_of(device)
    nat = native()
    nat.peer_fold(dev, stream, code, dcode, src_ptrs(bufs, ns), out.data_ptr() + (G + doff) * es, cnt, max_blocks)
    nat.peer_reduce(dev, stream, code, dcode, src_ptrs(bufs, ns), [ref.data_ptr() + (G + doff) * es], cnt)
    done(device)
    tag = (oname, dname, cnt, doff, ns, max_blocks)
    assert same(out, want), tag  # the CPU left fold, and the guards
    assert same(out, ref), (tag, "peer_reduce differs")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("oname,dname", PAIRS)
def test_peer_fold_grid(device, oname, dname):
    """Counts x destination offsets {0, 1, 3} elements x ns {1, 2, 3, 5, 8} x max_blocks {1, 0};
    the sources' 16-byte alignments differ from each other and from the destination's."""
    for cnt in COUNTS:
        for doff in (0, 1, 3):
            for ns in NS:
                for mb in (1, 0):
                    fold_case(device, oname, dname, cnt, doff, ns, mb)
    for k, b in enumerate(on_device(dname, device)):
        assert same(b, sources(dname)[k]), "source modified"


@pytest.mark.parametrize("device", DEVICES)
def test_peer_fold_every_other_pair_once(device):
    for oname, dname in OTHER_PAIRS:
        fold_case(device, oname, dname, 1031, 1, 3, 0)
    assert len(OTHER_PAIRS) + len(PAIRS) == 7 * 7 + 3 * 3
    nat, (dev, stream) = native(), dev_of(device)
    x = on_device("f32", device)
    with pytest.raises(Exception):  # a bitwise op on floats
        nat.peer_fold(dev, stream, 7, 0, [x[0].data_ptr()], x[1].data_ptr(), 4, 0)
    with pytest.raises(Exception):  # a destination that is not element-aligned
        nat.peer_fold(dev, stream, 0, 0, [x[0].data_ptr()], x[1].data_ptr() + 2, 4, 0)
    with pytest.raises(Exception):
        nat.peer_fold(dev, stream, 0, 0, [x[0].data_ptr()] * 9, x[1].data_ptr(), 4, 0)


# ------------------------------------------------------------------ peer_scan
def scan_case(device, oname, dname, cnt, ns, excl, inplace, max_blocks):
    dt = DT[dname]
    code, dcode = C._PR_OP_CODE[OPS[oname]], C._PR_DTYPES[dt]
    es = torch.empty(0, dtype=dt).element_size()
    pre = prefixes(oname, dname)
    nat, (dev, stream) = native(), dev_of(device)
    tag = (oname, dname, cnt, ns, excl, inplace, max_blocks)
    if inplace:
        work = [b.clone() for b in on_device(dname, device)[:ns]]
        ptrs = src_ptrs(work, ns)
        nat.peer_scan(dev, stream, code, dcode, excl, ptrs, ptrs, cnt, max_blocks)
        done(device)
        for j in range(ns):
            want = sources(dname)[j].clone()
            if not (excl and j == 0):  # (exclusive: source 0 keeps its values, they are the sentinel)
                want[SRC_OFFS[j]: SRC_OFFS[j] + cnt] = pre[j - 1 if excl else j][:cnt]
            assert same(work[j], want), (tag, j)
        last = work[ns - 1][SRC_OFFS[ns - 1]: SRC_OFFS[ns - 1] + cnt]
    else:
        bufs = on_device(dname, device)
        doffs = [(3 * j + 1) % 5 for j in range(ns)]  # destinations at differing alignments too
        guard = gen(dt, 78, G + 5 + NMAX + G)
        outs = [guard[: G + doffs[j] + cnt + G].clone().to(device) for j in range(ns)]
        nat.peer_scan(dev, stream, code, dcode, excl, src_ptrs(bufs, ns),
                      [outs[j].data_ptr() + (G + doffs[j]) * es for j in range(ns)], cnt, max_blocks)
        done(device)
        for j in range(ns):
            want = guard[: G + doffs[j] + cnt + G].clone()
            if not (excl and j == 0):  # dst[0] of the exclusive form keeps its sentinel
                want[G + doffs[j]: G + doffs[j] + cnt] = pre[j - 1 if excl else j][:cnt]
            assert same(outs[j], want), (tag, j)
        last = outs[ns - 1][G + doffs[ns - 1]: G + doffs[ns - 1] + cnt]
    # the last prefix is peer_reduce's result over the sources it folds, bit for bit
    nred = ns - 1 if excl else ns
    if nred >= 1:
        red = torch.zeros(cnt, dtype=dt).to(device)
        nat.peer_reduce(dev, stream, code, dcode, src_ptrs(on_device(dname, device), nred), [red.data_ptr()], cnt)
        done(device)
        assert same(last, red), (tag, "peer_reduce differs")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("oname,dname", PAIRS)
def test_peer_scan_grid(device, oname, dname):
    """Inclusive and exclusive, in place and out of place, counts x ns {1, 2, 3, 5, 8}, max_blocks
    {1, 0}: prefix j is the wide fold of sources 0..j rounded once."""
    for cnt in COUNTS:
        for ns in NS:
            for excl in (False, True):
                for inplace in (False, True):
                    for mb in ((1, 0) if cnt == 65541 or ns == 8 else (0,)):
                        scan_case(device, oname, dname, cnt, ns, excl, inplace, mb)
    for k, b in enumerate(on_device(dname, device)):
        assert same(b, sources(dname)[k]), "source modified"


@pytest.mark.parametrize("device", DEVICES)
def test_peer_scan_every_other_pair_once(device):
    for oname, dname in OTHER_PAIRS:
        scan_case(device, oname, dname, 1031, 3, False, True, 0)
        scan_case(device, oname, dname, 1031, 3, True, False, 0)


# ------------------------------------------------------------------ peer_reduce, vector body
VEC_PAIRS = PAIRS + [("PROD", "f16")]  # (the generator's zeros and negative values make exact -0 products)
VOFFS = [0, 1, 3]  # elements past a 16-byte boundary, the same for every pointer of a call


@functools.lru_cache(maxsize=None)
def shared_sources(dname, off):
    """The eight sources again (the operands of prefixes()), each moved to `off` elements past a
    16-byte boundary of a host buffer of its own, other values around them."""
    out = []
    for k, b in enumerate(sources(dname)):
        t = gen(DT[dname], 90 + k, off + NMAX + G)
        t[off: off + NMAX] = b[SRC_OFFS[k]: SRC_OFFS[k] + NMAX]
        out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def shared_on_device(dname, off, device):
    return tuple(b.clone().to(device) for b in shared_sources(dname, off))


@functools.lru_cache(maxsize=None)
def twin_reduce(oname, dname, ns):
    """peer_reduce's host twin (dev = -1) over all NMAX elements of the first ns sources; computed once."""
    dt = DT[dname]
    out = torch.zeros(NMAX, dtype=dt)
    native().peer_reduce(-1, 0, C._PR_OP_CODE[OPS[oname]], C._PR_DTYPES[dt],
                         [b.data_ptr() for b in shared_sources(dname, 0)[:ns]], [out.data_ptr()], NMAX)
    return out


def reduce_case(device, oname, dname, cnt, off, ns, nd, inplace):
    dt = DT[dname]
    code, dcode = C._PR_OP_CODE[OPS[oname]], C._PR_DTYPES[dt]
    host = shared_sources(dname, off)
    es = host[0].element_size()
    if inplace:  # dsts = srcs[:nd], on copies; what surrounds the range is the guard
        work = [b.clone() for b in shared_on_device(dname, off, device)[:ns]]
        outs, guards, at = work[:nd], host[:nd], off
        sp = [w.data_ptr() + off * es for w in work]
    else:
        work = shared_on_device(dname, off, device)[:ns]
        guard = gen(dt, 79, G + 3 + NMAX + G)[: G + off + cnt + G]
        outs, guards, at = [guard.clone().to(device) for _ in range(nd)], [guard] * nd, G + off
        sp = [w.data_ptr() + off * es for w in work]
    dp = [o.data_ptr() + at * es for o in outs]
    assert all(p % 16 == off * es % 16 for p in sp + dp)  # one offset within 16 bytes: the vector body
    dev, stream = dev_of(device)
    native().peer_reduce(dev, stream, code, dcode, sp, dp, cnt)
    done(device)
    tag = (oname, dname, cnt, off, ns, nd, inplace)
    for j in range(nd):
        want = guards[j].clone()
        want[at: at + cnt] = prefixes(oname, dname)[ns - 1][:cnt]
        assert same(outs[j], want), (tag, j)  # the CPU left fold, and the guards
        assert same(outs[j][at: at + cnt], twin_reduce(oname, dname, ns)[:cnt]), (tag, j, "host twin differs")
    for k in range(nd if inplace else 0, ns):
        assert same(work[k], host[k]), (tag, k, "source modified")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("oname,dname", VEC_PAIRS)
def test_peer_reduce_vector_body(device, oname, dname):
    """Every source and destination at one offset {0, 1, 3} elements past a 16-byte boundary, so
    that peer_reduce runs its vector body between a scalar head and tail: counts x ns {1, 2, 3, 5, 8}
    x nd {1, 3}, and in place (dsts = srcs[:3] of 5). Bitwise against the CPU left fold (wide
    accumulate, one rounding), guards included, and against the host twin."""
    for cnt in COUNTS:
        for off in VOFFS:
            for ns in NS:
                for nd in (1, 3):
                    reduce_case(device, oname, dname, cnt, off, ns, nd, False)
            reduce_case(device, oname, dname, cnt, off, 5, 3, True)
