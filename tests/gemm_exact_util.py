"""Helpers of tests/test_gemm_exact.py and tests/mp/gemm_exact_check.py: inputs whose GEMM
results are exact in fp32 whatever the order of the sums, guarded buffers, launches through
the raw bindings and fp64 CPU oracles.

A case is a dict; ``key(case)`` names it. ``gen_*`` builds its CPU inputs from a seed derived
from the key (the same values in every process), ``launch_*`` runs the kernel on the GPU and
returns CPU tensors (whole buffers, guards included, as integer bit patterns), ``check_*``
compares them with the fp64 oracle on the CPU. Nothing of mpit_amd.ops enters an oracle; the
fp16 plane builder only constructs inputs."""
import zlib

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
SENT32, SENT16 = 0x7FC5A5A5, 0x7FA5  # sentinel bit patterns (NaNs no kernel here produces)
PRE, POST, TAIL = 2, 3, 3            # guard rows before / after outputs, NaN rows after inputs

# gemm_nt paths: operand dtype, then how B (and A) reach the kernel
NT_PATHS = ("bf16", "f32", "f16b", "f16ab")
NT_K = {"bf16": (32, 64, 96, 160), "f32": (16, 48, 32, 96, 160), "f16b": (32, 96, 160), "f16ab": (32, 96, 160)}
WIDE_K = (32, 96, 160)
NT_M = (1, 31, 127, 128, 129, 257)
NT_N = (64, 128, 192)
EPI_KINDS = ("cin", "cin_alias", "cmask", "stats", "bnred", "bnred_nomask", "bnred2", "omax")
TN_PATHS = ("bf16", "f32", "f16x3")
TN_M = (1, 31, 32, 33, 255, 600, 10000)
TN_NK = ((64, 64), (128, 128), (192, 64), (64, 192))
# (Nb, H, W, C, Co, R, S, stride, pad)
CONV_SHAPES = ((2, 5, 9, 32, 64, 3, 3, 1, 1), (2, 7, 7, 96, 64, 3, 3, 1, 1), (3, 9, 6, 64, 128, 5, 5, 2, 2),
               (2, 8, 5, 64, 64, 1, 1, 2, 0), (2, 11, 11, 32, 64, 3, 3, 3, 1))


def key(c):
    return ",".join(f"{k}={c[k]}" for k in sorted(c))


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(key(c).encode()))


def dtype_of(path):
    return BF16 if path == "bf16" else F32


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def narrow(shape, g):
    """integers in [-3, 3]: one plane in bf16 and in fp16"""
    return ints(shape, -3, 3, g)


def wide(shape, g):
    """4 i + j 2^-10, i in [-3, 3], j in [-15, 15]: 14 significant bits, granularity 2^-10"""
    return 4.0 * ints(shape, -3, 3, g) + ints(shape, -15, 15, g) * 2.0 ** -10


def assert_exact(a, b, gran, what=""):
    """Every partial sum of a . b^T (any order) is a multiple of gran below 2^24 gran."""
    for t, gt in ((a, gran[0]), (b, gran[1])):
        q = t.double() / gt
        assert torch.equal(q, q.round()), f"{what}: operand off its granularity"
    top = (a.abs().double() @ b.abs().double().t()).max().item() / (gran[0] * gran[1])
    assert top < 2 ** 24, f"{what}: |A||B|^T reaches {top} units, not exact in fp32"
    return top


# ------------------------------------------------------------------ buffers
def in_buf(t, ld, dt, dev, tail=TAIL):
    """t [rows, cols] inside a [rows + tail, ld] allocation, padding columns and tail rows NaN"""
    rows, cols = t.shape
    buf = torch.full((rows + tail, ld), float("nan"), dtype=dt)
    buf[:rows, :cols] = t.to(dt)
    return buf.to(dev)


def out_buf(rows, ld, dt, dev, pre=PRE, post=POST):
    """[pre + rows + post, ld] of sentinel bits (integer view) and the pointer of row `pre`"""
    idt, sent, esz = (torch.int16, SENT16, 2) if dt == BF16 else (torch.int32, SENT32, 4)
    full = torch.full((pre + rows + post, ld), sent, dtype=idt, device=dev)
    return full, full.data_ptr() + pre * ld * esz


def owned(full, rows, cols, dt, pre=PRE):
    """the region a call owns, as values"""
    return full[pre:pre + rows, :cols].contiguous().view(dt)


def assert_guards(full, rows, cols, what, pre=PRE):
    """everything outside [pre, pre + rows) x [0, cols) is still the sentinel"""
    sent = SENT16 if full.dtype == torch.int16 else SENT32
    out = torch.ones(full.shape, dtype=torch.bool)
    out[pre:pre + rows, :cols] = False
    bad = out & (full != sent)
    assert not bad.any(), f"{what}: {int(bad.sum())} guard elements written, first at {bad.nonzero()[0].tolist()}"


def same_bits(got, ref, what):
    idt = torch.int16 if ref.dtype == BF16 else torch.int32
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if not torch.equal(got.view(idt), ref.view(idt)):
        bad = got.view(idt) != ref.view(idt)
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: "
                             f"got {got[i].item()!r} want {ref[i].item()!r}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bound(t, dev):
    """slotted device bound (kernels.h kBoundFloats) holding max |t|"""
    from mpit_amd.ops.conv import bound_of_value

    return bound_of_value(t.abs().max().reshape(1).float().to(dev))


def _planes(buf, bnd):
    from mpit_amd.ops.conv import f16_planes

    return f16_planes(buf.reshape(-1), bnd)


# ------------------------------------------------------------------ gemm_nt, plain (+ stats)
def nt_cases(paths=NT_PATHS, ms=NT_M):
    out = []
    for p in paths:
        for K in NT_K[p]:
            for N in NT_N:
                for M in ms:
                    out.append(dict(op="nt", path=p, M=M, N=N, K=K, fam="narrow", tight=0))
                    if p != "bf16" and K in WIDE_K:
                        out.append(dict(op="nt", path=p, M=M, N=N, K=K, fam="wideA", tight=0))
                        out.append(dict(op="nt", path=p, M=M, N=N, K=K, fam="wideB", tight=0))
        out.append(dict(op="nt", path=p, M=129, N=192, K=96, fam="narrow", tight=1))
    return out


def nt256_cases():
    """bf16, K = 2304, N % 128 == 0: nt_tile_config's deep-K rule picks 256 x 128 blocks"""
    return [dict(op="nt", path="bf16", M=M, N=N, K=2304, fam="narrow", tight=0, stats=s)
            for M in (255, 257, 513) for N in (128, 256) for s in (0, 1)]


def gen_nt(c):
    g = _gen(c)
    M, N, K = c["M"], c["N"], c["K"]
    a = wide((M, K), g) if c["fam"] == "wideA" else narrow((M, K), g)
    b = wide((N, K), g) if c["fam"] == "wideB" else narrow((N, K), g)
    gran = (2.0 ** -10 if c["fam"] == "wideA" else 1.0, 2.0 ** -10 if c["fam"] == "wideB" else 1.0)
    assert_exact(a, b, gran, key(c))
    return a, b


def pz(t):
    """-0 -> +0: a sum that starts from a zero accumulator is never -0, whereas a library product
    of a single term (M or K of 1) may be"""
    return t + 0.0


def ref_nt(a, b, dt):
    r = pz(a.double() @ b.double().t()).float()
    return r.to(BF16) if dt == BF16 else r


def _nt_operands(c, a, b, dev, lda, ldb):
    """device operands of a path: (keep-alive list, A pointer, B pointer, kwargs)"""
    dt = dtype_of(c["path"])
    A, B = in_buf(a, lda, dt, dev), in_buf(b, ldb, dt, dev)
    keep, kw = [A, B], dict(f32=dt == F32)
    pa, pb = A.data_ptr(), B.data_ptr()
    if c["path"] in ("f16b", "f16ab"):
        ab, bb = _bound(a, dev), _bound(b, dev)
        Bp = _planes(B, bb)
        keep += [ab, bb, Bp]
        kw.update(bps=Bp[0].numel(), amax_a=ab.data_ptr(), amax_b=bb.data_ptr())
        pb = Bp.data_ptr()
        if c["path"] == "f16ab":
            Ap = _planes(A, ab)
            keep.append(Ap)
            kw["aps"] = Ap[0].numel()
            pa = Ap.data_ptr()
    return keep, pa, pb, kw


def launch_nt(m, c, dev="cuda"):
    a, b = gen_nt(c)
    M, N, K = c["M"], c["N"], c["K"]
    dt = dtype_of(c["path"])
    lda, ldb, ldc = (K, K, N) if c["tight"] else (K + 8, K + 16, N + 8)
    keep, pa, pb, kw = _nt_operands(c, a, b, dev, lda, ldb)
    full, pc = out_buf(M, ldc, dt, dev)
    res, ps = {}, 0
    if c.get("stats"):
        nt = m.gemm_nt_tiles(M)
        assert m.gemm_nt_stats_floats(M, N) == nt * 2 * N
        sfull, ps = out_buf(nt, 2 * N, F32, dev)
    m.gemm_nt(0, _stream(), M, N, K, pa, lda, pb, ldb, pc, ldc, ps, **kw)
    torch.cuda.synchronize()
    res["C"] = full.cpu()
    if c.get("stats"):
        res["stats"] = sfull.cpu()
    del keep
    return res


def check_stats(sfull, cd, M, N, what, pre=PRE):
    """per-128-row-tile (mean, M2) against fp64 over the stored C (tolerances of
    tests/test_gemm.py::test_gemm_nt_tile_stats_large_mean); a one-row tile has M2 == 0"""
    nt = (M + 127) // 128
    assert_guards(sfull, nt, 2 * N, what + " stats", pre)
    p = owned(sfull, nt, 2 * N, F32, pre).view(nt, 2, N).double()
    for t in range(nt):
        rows = cd[128 * t:min(M, 128 * t + 128)]
        n = rows.shape[0]
        torch.testing.assert_close(p[t, 0], rows.mean(0), rtol=1e-7, atol=1e-4, msg=lambda s: f"{what} tile {t} mean: {s}")
        torch.testing.assert_close(p[t, 1] / n, rows.var(0, unbiased=False), rtol=1e-4, atol=1e-5,
                                   msg=lambda s: f"{what} tile {t} var: {s}")
        if n == 1:
            assert (p[t, 1] == 0).all(), f"{what}: one-row tile {t} has M2 != 0"


def check_nt(c, res):
    a, b = gen_nt(c)
    M, N = c["M"], c["N"]
    dt = dtype_of(c["path"])
    what = key(c)
    assert_guards(res["C"], M, N, what)
    got = owned(res["C"], M, N, dt)
    same_bits(got, ref_nt(a, b, dt), what)
    if c.get("stats"):  # (M = 257: three partial rows, the last over one row)
        check_stats(res["stats"], got.double(), M, N, what)


# ------------------------------------------------------------------ gemm_nt epilogues
def epi_cases(ms=(1, 129, 257)):
    return [dict(op="epi", path=p, epi=e, M=M, N=N, K=K)
            for p in ("bf16", "f32") for e in EPI_KINDS for N in NT_N for M in ms for K in (32, 96)]


def unpack_mask(mask, M, N):
    """[M, N] 0/1 of the bn_act bit mask: one byte per 8 channels, bit e = channel 8k + e"""
    by = mask[:M * N // 8].to(torch.int32)
    bits = (by[:, None] >> torch.arange(8, dtype=torch.int32)[None, :]) & 1
    return bits.reshape(M, N).double()


def gen_epi(c):
    g = _gen(c)
    M, N, K = c["M"], c["N"], c["K"]
    d = {}
    # bf16 cin cases: sixteenths, so that the product itself rounds when it is stored as bf16
    frac = c["path"] == "bf16" and c["epi"] in ("cin", "cin_alias")
    sc = 1.0 / 16 if frac else 1.0
    d["a"] = ints((M, K), -32 if frac else -2, 32 if frac else 2, g) * sc
    d["b"] = ints((N, K), -32 if frac else -2, 32 if frac else 2, g) * sc
    assert_exact(d["a"], d["b"], (sc, sc), key(c))
    if c["epi"] in ("cin", "cin_alias", "cmask"):
        d["cin"] = ints((M, N), -64 if frac else -3, 64 if frac else 3, g) * sc
    if c["epi"] == "cmask":
        d["cmask"] = torch.randint(0, 256, (M * N // 8,), generator=g).to(torch.uint8)
    if c["epi"] in ("bnred", "bnred_nomask", "bnred2"):
        d["x"] = narrow((M, N), g)
        d["mean"] = ints((N,), -8, 8, g) / 4
        if c["epi"] != "bnred_nomask":
            d["mask"] = torch.randint(0, 256, (M * N // 8,), generator=g).to(torch.uint8)
        if c["epi"] == "bnred2":
            d["x2"] = narrow((M, N), g)
            d["mean2"] = ints((N,), -8, 8, g) / 4
    return d


def epi_oracle(c, d):
    """(stored C, dict of partial oracles), everything from fp64"""
    M, N = c["M"], c["N"]
    dt = dtype_of(c["path"])
    P = pz(d["a"].double() @ d["b"].double().t())
    o = {}
    zero = torch.zeros((), dtype=torch.float64)
    if "cin" in d:
        bits = unpack_mask(d["cmask"], M, N) if "cmask" in d else torch.ones(M, N, dtype=torch.float64)
        if dt == BF16:  # the kernel rounds the product to bf16, adds cin, rounds again
            c1 = P.float().to(BF16)
            s = c1.double() + torch.where(bits > 0, d["cin"].double(), zero)
            assert torch.equal(s.float().double(), s)
            C = s.float().to(BF16)
            if c["epi"] != "cmask" and M > 1:
                once = (P + d["cin"].double()).float().to(BF16)
                assert not torch.equal(C, once), "cin does not tell the two roundings apart"
        else:
            C = (P + torch.where(bits > 0, d["cin"].double(), zero)).float()
    else:
        C = P.float().to(dt)
    if c["epi"].startswith("bnred"):
        bits = unpack_mask(d["mask"], M, N) if "mask" in d else torch.ones(M, N, dtype=torch.float64)
        dz = torch.where(bits > 0, C.double(), zero)
        nt = (M + 127) // 128
        xm = d["x"].double() - d["mean"].double()
        top = (dz.abs() * xm.abs() * 4).view(-1, N)
        assert max(top[128 * t:128 * t + 128].sum(0).max().item() for t in range(nt)) < 2 ** 24
        part = torch.stack([torch.stack([dz[128 * t:128 * t + 128].sum(0), (dz * xm)[128 * t:128 * t + 128].sum(0)])
                            for t in range(nt)])
        o["part"] = pz(part).float()
        if "x2" in d:
            xm2 = d["x2"].double() - d["mean2"].double()
            o["part2"] = (torch.stack([torch.stack([dz[128 * t:128 * t + 128].sum(0),
                                                   (dz * xm2)[128 * t:128 * t + 128].sum(0)]) for t in range(nt)]) + 0.0).float()
    return C, o


ROW0 = 3
OEPOCH = 7


def launch_epi(m, c, dev="cuda"):
    d = gen_epi(c)
    M, N, K, e = c["M"], c["N"], c["K"], c["epi"]
    dt = dtype_of(c["path"])
    lda, ldb = K + 8, K + 16
    ldc = N if e in ("cmask", "bnred", "bnred_nomask", "bnred2") else N + 8
    A, B = in_buf(d["a"], lda, dt, dev), in_buf(d["b"], ldb, dt, dev)
    full, pc = out_buf(M, ldc, dt, dev)
    kw, keep, res = dict(f32=dt == F32), [], {}
    nt = m.gemm_nt_tiles(M)
    if e == "cin_alias":  # cin lives in C: the owned region starts as cin, the guards as sentinel
        full[PRE:PRE + M, :N] = d["cin"].to(dt).view(full.dtype).to(dev)
        kw["cin"] = pc
    elif e in ("cin", "cmask"):
        cin = in_buf(d["cin"], ldc, dt, dev)
        keep.append(cin)
        kw["cin"] = cin.data_ptr()
        if e == "cmask":
            cm = torch.cat([d["cmask"], torch.zeros(64, dtype=torch.uint8)]).to(dev)
            keep.append(cm)
            kw["cmask"] = cm.data_ptr()
    elif e == "stats":
        sfull, ps = out_buf(nt, 2 * N, F32, dev)
        kw["stats"] = ps
    elif e == "omax":
        om = torch.full((m.bound_floats(),), SENT32, dtype=torch.int32, device=dev)
        slots = om.view(16, 32)
        slots[:, 0] = torch.tensor([1e9]).view(torch.int32).item()  # an older launch's larger maximum
        slots[:, 1] = OEPOCH - 1
        kw.update(omax=om.data_ptr(), oepoch=OEPOCH)
    else:
        x = in_buf(d["x"], N, dt, dev)
        mean = d["mean"].to(dev)
        pfull, _ = out_buf(nt, 2 * N, F32, dev, pre=ROW0)
        keep += [x, mean]
        kw.update(red_part=pfull.data_ptr(), red_x=x.data_ptr(), red_mean=mean.data_ptr(), red_row0=ROW0)
        if "mask" in d:
            mk = torch.cat([d["mask"], torch.zeros(64, dtype=torch.uint8)]).to(dev)
            keep.append(mk)
            kw["red_mask"] = mk.data_ptr()
        if e == "bnred2":
            x2 = in_buf(d["x2"], N, dt, dev)
            mean2 = d["mean2"].to(dev)
            p2full, _ = out_buf(nt, 2 * N, F32, dev, pre=ROW0)
            keep += [x2, mean2]
            kw.update(red_part2=p2full.data_ptr(), red_x2=x2.data_ptr(), red_mean2=mean2.data_ptr())
    m.gemm_nt(0, _stream(), M, N, K, A.data_ptr(), lda, B.data_ptr(), ldb, pc, ldc, **kw)
    torch.cuda.synchronize()
    res["C"] = full.cpu()
    if e == "stats":
        res["stats"] = sfull.cpu()
    if e == "omax":
        res["omax"] = om.cpu()
    if e.startswith("bnred"):
        res["part"] = pfull.cpu()
        if e == "bnred2":
            res["part2"] = p2full.cpu()
    del keep
    return res


def check_epi(c, res):
    d = gen_epi(c)
    M, N, e = c["M"], c["N"], c["epi"]
    dt = dtype_of(c["path"])
    what = key(c)
    C, o = epi_oracle(c, d)
    assert_guards(res["C"], M, N, what)
    got = owned(res["C"], M, N, dt)
    same_bits(got, C, what)
    nt = (M + 127) // 128
    if e == "stats":
        check_stats(res["stats"], got.double(), M, N, what)
    for name in ("part", "part2"):
        if name in o:
            assert_guards(res[name], nt, 2 * N, f"{what} {name}", pre=ROW0)
            same_bits(owned(res[name], nt, 2 * N, F32, pre=ROW0).view(nt, 2, N), o[name], f"{what} {name}")
    if e == "omax":
        slots = res["omax"].view(16, 32)
        assert (slots[:, 2:] == SENT32).all(), f"{what}: omax wrote outside its slots"
        ours = slots[:, 1] == OEPOCH
        old = ~ours
        assert ours.any() and (slots[old, 1] == OEPOCH - 1).all(), f"{what}: omax epochs {slots[:, 1].tolist()}"
        assert (slots[old, 0].contiguous().view(F32) == 1e9).all(), f"{what}: a stale slot changed"
        top = slots[ours, 0].contiguous().view(F32).max().item()
        assert top == C.float().abs().max().item(), (what, top, C.float().abs().max().item())


# ------------------------------------------------------------------ gemm_tn
def tn_cases(ms=TN_M):
    return [dict(op="tn", path=p, M=M, N=N, K=K, beta=be)
            for p in TN_PATHS for (N, K) in TN_NK for M in ms for be in (0, 1)]


def gen_tn(c):
    g = _gen(c)
    M, N, K = c["M"], c["N"], c["K"]
    y, x = narrow((M, N), g), narrow((M, K), g)
    base = ints((N, K), -50, 50, g)
    top = assert_exact(y.t(), x.t(), (1.0, 1.0), key(c))
    assert top + 50 < 2 ** 24
    return y, x, base


def launch_tn(m, c, dev="cuda"):
    y, x, base = gen_tn(c)
    M, N, K, beta = c["M"], c["N"], c["K"], c["beta"]
    dt = BF16 if c["path"] == "bf16" else F32
    ldy, ldx = N + 8, K + 8
    Y, X = in_buf(y, ldy, dt, dev), in_buf(x, ldx, dt, dev)
    full, po = out_buf(N, K, F32, dev)
    if beta:
        full[PRE:PRE + N] = base.view(torch.int32).to(dev)
    nws = m.gemm_tn_ws_floats(0, M, N, K)
    # the plan this case is meant to hit (a device whose CU count changes it fails here)
    if M <= 255:
        assert nws == 0, (key(c), nws)
    elif M == 600:
        assert nws % (N * K) == 0 and 2 <= nws // (N * K) <= 32, (key(c), nws)
    elif (N, K) == (64, 64):
        assert nws // (N * K) > 33, (key(c), nws)  # > 32 partials plus their group sums: two levels
    else:
        assert nws >= 2 * N * K, (key(c), nws)
    # (a single split with beta = 1 goes through the reduce on one N x K partial)
    ws = torch.zeros(max(nws, N * K) + 4 * N * K, dtype=F32, device=dev)
    kw, keep = dict(f32=dt == F32), []
    if c["path"] == "f16x3":
        keep = [_bound(y, dev), _bound(x, dev)]
        kw.update(amax_y=keep[0].data_ptr(), amax_x=keep[1].data_ptr())
    m.gemm_tn(0, _stream(), M, N, K, Y.data_ptr(), ldy, X.data_ptr(), ldx, po, ws.data_ptr(), float(beta), **kw)
    torch.cuda.synchronize()
    del keep
    return {"out": full.cpu()}


def check_tn(c, res):
    y, x, base = gen_tn(c)
    N, K = c["N"], c["K"]
    ref = pz(y.double().t() @ x.double())
    if c["beta"]:
        ref = ref + base.double()
    assert_guards(res["out"], N, K, key(c))
    same_bits(owned(res["out"], N, K, F32), ref.float(), key(c))


# ------------------------------------------------------------------ convolutions
def conv_cases():
    out = []
    for p in ("bf16", "f32"):
        for i, s in enumerate(CONV_SHAPES):
            C, st = s[3], s[7]
            for v in ("plain", "bias_relu", "cin"):
                out.append(dict(op="conv", path=p, shape=i, var=v))
            if i == 0:
                out.append(dict(op="conv", path=p, shape=i, var="relub"))
            # conv_dgrad_strided: 2 <= stride <= 4 and C % 64 == 0; conv_wgrad: C % 64 == 0
            if st > 1 and C % 64 == 0:
                out.append(dict(op="conv", path=p, shape=i, var="dgrad"))
            if C % 64 == 0:
                out.append(dict(op="conv", path=p, shape=i, var="wgrad0"))
                out.append(dict(op="conv", path=p, shape=i, var="wgrad1"))
    return out


def conv_out_hw(s):
    Nb, H, W, C, Co, R, S, st, pad = s
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


def gen_conv(c):
    g = _gen(dict(op="conv", shape=c["shape"]))  # one data set per shape, shared by its variants
    s = CONV_SHAPES[c["shape"]]
    Nb, H, W, C, Co, R, S, st, pad = s
    Ho, Wo = conv_out_hw(s)
    d = dict(x=narrow((Nb, H, W, C), g), w=narrow((Co, R, S, C), g), dy=narrow((Nb, Ho, Wo, Co), g),
             bias=ints((Co,), -8, 8, g), cin=narrow((Nb, Ho, Wo, Co), g), yrelu=narrow((Nb, Ho, Wo, Co), g),
             base=ints((Co, R, S, C), -50, 50, g))
    assert 9 * max(R * S * C, R * S * Co, Nb * Ho * Wo) + 60 < 2 ** 24
    return d


_CONV_REF = {}


def conv_ref(i):
    """fp64 F.conv2d and its autograd, once per shape: (y, dx, dw) in NHWC / [Co][R][S][C]"""
    if i not in _CONV_REF:
        s = CONV_SHAPES[i]
        st, pad = s[7], s[8]
        d = gen_conv(dict(shape=i))
        x = d["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
        w = d["w"].double().permute(0, 3, 1, 2).requires_grad_(True)
        y = F.conv2d(x, w, stride=st, padding=pad)
        y.backward(d["dy"].double().permute(0, 3, 1, 2))
        _CONV_REF[i] = (pz(y.detach().permute(0, 2, 3, 1).contiguous()), pz(x.grad.permute(0, 2, 3, 1).contiguous()),
                        pz(w.grad.permute(0, 2, 3, 1).contiguous()))
    return _CONV_REF[i]


def _img_buf(t, dt, dev, guard):
    """NHWC tensor as [pixels, channels] rows with `guard` NaN pixels before and after"""
    ch = t.shape[-1]
    rows = t.reshape(-1, ch)
    buf = torch.full((guard + rows.shape[0] + guard, ch), float("nan"), dtype=dt)
    buf[guard:guard + rows.shape[0]] = rows.to(dt)
    buf = buf.to(dev)
    return buf, buf.data_ptr() + guard * ch * (2 if dt == BF16 else 4)


def launch_conv(m, c, dev="cuda"):
    d = gen_conv(c)
    s = CONV_SHAPES[c["shape"]]
    Nb, H, W, C, Co, R, S, st, pad = s
    Ho, Wo = conv_out_hw(s)
    dt = dtype_of(c["path"])
    f32 = dt == F32
    v = c["var"]
    M = Nb * Ho * Wo
    G = 8  # guard pixels
    res = {}
    if v in ("plain", "bias_relu", "cin", "relub"):
        assert m.conv_supported(C, Co)
        xb, px = _img_buf(d["x"], dt, dev, G)
        wb = in_buf(d["w"].reshape(Co, -1), R * S * C, dt, dev)
        full, py = out_buf(M, Co, dt, dev, pre=G, post=G)
        kw, keep = dict(f32=f32), []
        if v == "bias_relu":
            keep.append(d["bias"].to(dev))
            kw.update(bias=keep[0].data_ptr(), relu=True)
        if v == "cin":
            keep.append(in_buf(d["cin"].reshape(M, Co), Co, dt, dev))
            kw["cin"] = keep[0].data_ptr()
        if v == "relub":
            nt = m.gemm_nt_tiles(M)
            keep.append(in_buf(d["yrelu"].reshape(M, Co), Co, dt, dev))
            pfull, pp = out_buf(nt, 2 * Co, F32, dev)
            kw.update(red_part=pp, red_x=keep[0].data_ptr(), red_relu=True)
        m.conv_fwd(0, _stream(), Nb, H, W, C, Co, R, S, st, pad, px, wb.data_ptr(), py, **kw)
        torch.cuda.synchronize()
        res["y"] = full.cpu()
        if v == "relub":
            res["part"] = pfull.cpu()
    elif v == "dgrad":
        w32 = d["w"].to(dev)
        wbf = torch.empty(Co, R, S, C, dtype=BF16, device=dev)
        wc = torch.empty(m.conv_dgrad_strided_wfloats(C, Co, R, S, st, pad), dtype=dt, device=dev)
        m.conv_dgrad_strided_weights(0, _stream(), w32.data_ptr(), Co, C, R, S, st, pad, 0 if f32 else wbf.data_ptr(),
                                     wc.data_ptr(), f32=f32)
        yb, py = _img_buf(d["dy"], dt, dev, G)
        full, pdx = out_buf(Nb * H * W, C, dt, dev, pre=G, post=G)
        m.conv_dgrad_strided(0, _stream(), Nb, H, W, C, Co, R, S, st, pad, py, wc.data_ptr(), pdx, f32=f32)
        torch.cuda.synchronize()
        res["dx"] = full.cpu()
    else:
        beta = float(v == "wgrad1")
        xb, px = _img_buf(d["x"], dt, dev, G)
        yb, py = _img_buf(d["dy"], dt, dev, G)
        full, pdw = out_buf(Co, R * S * C, F32, dev)
        if beta:
            full[PRE:PRE + Co] = d["base"].reshape(Co, -1).view(torch.int32).to(dev)
        nws = m.conv_wgrad_ws_floats(0, Nb, H, W, C, Co, R, S, st, pad)
        ws = torch.zeros(max(nws, Co * R * S * C) + 4 * Co * R * S * C, dtype=F32, device=dev)
        m.conv_wgrad(0, _stream(), Nb, H, W, C, Co, R, S, st, pad, py, px, pdw, ws.data_ptr(), beta, f32=f32)
        torch.cuda.synchronize()
        res["dw"] = full.cpu()
    return res


def check_conv(c, res):
    d = gen_conv(c)
    s = CONV_SHAPES[c["shape"]]
    Nb, H, W, C, Co, R, S, st, pad = s
    Ho, Wo = conv_out_hw(s)
    dt = dtype_of(c["path"])
    v, what = c["var"], key(c)
    M = Nb * Ho * Wo
    y64, dx64, dw64 = conv_ref(c["shape"])
    G = 8
    if v in ("plain", "bias_relu", "cin", "relub"):
        P = y64.reshape(M, Co)
        if v == "bias_relu":
            ref = (P + d["bias"].double()).clamp(min=0).float().to(dt)
        elif v == "cin":
            # bf16: the product is rounded, cin added, the sum rounded again
            ref = (P.float().to(dt).double() + d["cin"].reshape(M, Co).double()).float().to(dt)
        elif v == "relub":
            ref = torch.where(d["yrelu"].reshape(M, Co) > 0, P, torch.zeros((), dtype=torch.float64)).float().to(dt)
        else:
            ref = P.float().to(dt)
        assert_guards(res["y"], M, Co, what, pre=G)
        got = owned(res["y"], M, Co, dt, pre=G)
        same_bits(got, ref, what)
        if v == "relub":
            nt = (M + 127) // 128
            sums = torch.stack([ref.double()[128 * t:128 * t + 128].sum(0) for t in range(nt)]).float()
            part = res["part"]
            # row 0 of every tile's pair holds the column sums; the second row is not written
            own = owned(part, nt, 2 * Co, F32).view(nt, 2, Co)
            same_bits(own[:, 0].contiguous(), sums, what + " part")
            keep = part.clone()
            keep[PRE:PRE + nt, :Co] = SENT32
            assert (keep == SENT32).all(), what + ": relub partials wrote outside their rows"
    elif v == "dgrad":
        assert_guards(res["dx"], Nb * H * W, C, what, pre=G)
        same_bits(owned(res["dx"], Nb * H * W, C, dt, pre=G), dx64.reshape(-1, C).float().to(dt), what)
    else:
        ref = dw64.reshape(Co, -1)
        if v == "wgrad1":
            ref = ref + d["base"].reshape(Co, -1).double()
        assert_guards(res["dw"], Co, R * S * C, what)
        same_bits(owned(res["dw"], Co, R * S * C, F32), ref.float(), what)


# ------------------------------------------------------------------ dispatch
LAUNCH = {"nt": launch_nt, "epi": launch_epi, "tn": launch_tn, "conv": launch_conv}
CHECK = {"nt": check_nt, "epi": check_epi, "tn": check_tn, "conv": check_conv}


def worker_cases(env):
    """The reduced list the variant worker runs under the knobs `env` sets."""
    ms = (1, 129, 257)
    paths = NT_PATHS
    # nt_plan: "pre-split B planes need the fp32 bf16x6 path with K % 32 == 0" — the native
    # fp32 MFMA and the 16-deep k-tile builds have no planes kernels
    if env.get("MPIT_F32_MFMA") == "native" or env.get("MPIT_F32_BK") == "16":
        paths = ("bf16", "f32")
    cases = nt_cases(paths, ms) + epi_cases(ms) + tn_cases((1, 33, 600, 10000))
    if env.get("MPIT_GEMM_TILE") == "256":  # 256 x 256 tiles need N % 256 == 0 and K % 64 == 0
        cases += [dict(op="nt", path="bf16", M=M, N=256, K=K, fam="narrow", tight=0) for M in ms for K in (64, 128)]
    if env.get("MPIT_GEMM_STAGES"):  # K = 128: exactly four k-tiles on the 4-deep bf16 ring
        cases += [dict(op="nt", path="bf16", M=M, N=N, K=128, fam="narrow", tight=0) for M in ms for N in NT_N]
    return cases
