"""Helpers of tests/test_bn_exact.py and tests/mp/bn_exact_check.py: the fused BatchNorm kernels
(csrc/kernels/bn_act.hip) through the raw bindings against fp64 CPU oracles written from the
documented formulas.

A case is a dict; ``key(case)`` names it. ``gen_*`` builds its CPU inputs from a seed derived
from the key and asserts the exactness bound the case relies on, ``launch_*`` runs the kernels
and returns CPU tensors (whole buffers, guards included, as integer bit patterns), ``check_*``
compares them with the oracle on the CPU. Inputs carry NaN tail rows, every output sits between
sentinel guard rows, the workspace ends in sentinels. Nothing of mpit_amd.ops enters an oracle.

The oracle (fp64): mean and biased variance over the M rows, rstd = 1/sqrt(var + eps),
scale = gamma rstd, shift = beta - mean scale, running stats with momentum and the unbiased
factor M/(M-1) (M/1 for M = 1), t = x scale + shift (+ res), ReLU, mask bit v of byte
row C/8 + c/8 = (t > 0) for channel 8 (c/8) + v; backward dz = dy mask, dbeta = sum dz,
dgamma = rstd sum dz (x - mean), A = gamma rstd, Cc = -A rstd^2 mean(dz (x - mean)),
B = -A mean(dz) - Cc mean, dx = A dz + Cc x + B, dres = dz."""
import zlib

import torch

from gemm_exact_util import (BF16, F32, PRE, SENT32, assert_guards, in_buf, ints, key, out_buf, owned, same_bits,
                             unpack_mask, wide)

MOM = float(torch.tensor(0.1, dtype=F32))   # the fp32 values the kernels receive
EPS = float(torch.tensor(1e-5, dtype=F32))
NSLOT, SSTRIDE = 16, 32                     # kernels.h kBoundSlots, kBoundStride
ABOVE, BELOW = 2.0 ** 20, 2.0 ** -10        # pre-filled amax slots: above every output / below every block's maximum
BSENT, BPRE, BPOST = 0xA5, 64, 96           # mask bytes: sentinel and guard bytes before / after
WPRE, WPOST = 64, 256                       # workspace: sentinel floats before / after
TILE = 128                                  # rows per GEMM statistics tile (bn_act.hip kTileRows)


def dt_of(c):
    return BF16 if c["dt"] == "bf16" else F32


def off_of(c):
    """common offset of the integer data: |mean| >> std, yet every value exact in its type"""
    return 100.0 if c["dt"] == "bf16" else 1000.0


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(key(c).encode()))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def cached(fn):
    """remembers the case generated last: launch_* and check_* of one case share one generation"""
    last = []

    def wrap(c):
        k = key(c)
        if not last or last[0] != k:
            last[:] = [k, fn(c)]
        return last[1]
    return wrap


# ------------------------------------------------------------------ number helpers
def exact32(v, what):
    """v (fp64) is an fp32 number: the fp32 operation that produces it does not round"""
    assert torch.equal(v.float().double(), v), f"{what}: not exact in fp32"
    return v


def bf16_ties(v):
    """elements exactly half way between two bf16 numbers (9 significant bits, the last one set)"""
    m, _ = torch.frexp(v.abs())
    q = m * 512
    return (q == q.round()) & (q.remainder(2) == 1)


def ulp(v, bits=24):
    """spacing of the floats with `bits` significant bits at |v| (fp32 24, bf16 8); 0 at 0"""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - bits))


def assert_within(got, ref, terms, nround, what, bits=24, extra=0.0):
    """|got - ref| <= (nround + 1) ulp of the largest-magnitude term: nround roundings in the
    kernel's expression, each at most one ulp of the largest term, plus one (extra: a derived
    bound of the error an inexact input of the expression brings in)"""
    big = torch.stack([t.abs().expand_as(ref) for t in terms]).amax(0)
    tol = (nround + 1) * ulp(big, bits) + extra
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} beyond {nround + 1} ulp, first at {i}: got "
                             f"{got[i].item()!r} want {ref[i].item()!r} (err {err[i].item():.3e}, tol {tol[i].item():.3e})")


def pack_mask(pos):
    """[M, C] booleans -> the bit mask bytes: bit v of byte row C/8 + c/8 is channel 8 (c/8) + v"""
    M, C = pos.shape
    w = 1 << torch.arange(8, dtype=torch.int32)
    return (pos.view(M, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)


# ------------------------------------------------------------------ the oracle
def bn_coefs64(mean, var, M, gamma, beta, rmean0, rvar0):
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma * rstd
    o = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale)
    o["rmean"] = (1.0 - MOM) * rmean0 + MOM * mean
    o["unb"] = var * M / max(M - 1, 1)
    o["rvar"] = (1.0 - MOM) * rvar0 + MOM * o["unb"]
    return o


def bn_forward64(x, gamma, beta, rmean0, rvar0, res=None, relu=True):
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    o = bn_coefs64(mean, var, x.shape[0], gamma, beta, rmean0, rvar0)
    t = x * o["scale"] + o["shift"]
    if res is not None:
        t = t + res
    o["pos"] = t > 0
    o["y"] = t.clamp(min=0) if relu else t
    return o


def bn_bwd_coefs64(s1, s2, M, gamma, mean, rstd):
    """from s1 = sum dz and s2 = sum dz (x - mean)"""
    A = gamma * rstd
    Cc = -A * rstd ** 2 * (s2 / M)
    return dict(dbeta=s1, dgamma=rstd * s2, A=A, Cc=Cc, t1=A * (s1 / M), t2=Cc * mean, B=-A * (s1 / M) - Cc * mean,
                mean=mean, rstd=rstd)


def bn_backward64(dy, pos, x, gamma, mean, rstd):
    dz = dy if pos is None else dy * pos
    o = bn_bwd_coefs64(dz.sum(0), (dz * (x - mean)).sum(0), x.shape[0], gamma, mean, rstd)
    o["dres"] = dz
    o["dx"] = o["A"] * dz + o["Cc"] * x + o["B"]
    return o


# fp32 roundings of the kernels' expressions (fin_fwd_channel / fin_bwd_channel), and the terms
# whose largest magnitude scales the ulp. The sums behind them are exact (asserted per case) and
# combined in fp64, so nothing else rounds.
#   save_mean = float(mean)                                  1
#   save_rstd = float(1 / sqrt(var + eps))                   1
#   scale     = gamma * rstd                                 rstd 1, product 1                  = 2
#   shift     = beta - float(mean) * scale                   mean 1, scale 2, product 1, sub 1  = 5
#   rmean     = (1 - mom) * rmean + mom * float(mean)        1 - mom 1, product 1, mean 1, product 1, add 1 = 5
#   rvar      = (1 - mom) * rvar + mom * float(unbiased)     likewise                           = 5
def check_fwd_coefs(got, o, rmean0, rvar0, what):
    assert_within(got["save_mean"], o["mean"], [o["mean"]], 1, what + " save_mean")
    assert_within(got["save_rstd"], o["rstd"], [o["rstd"]], 1, what + " save_rstd")
    assert_within(got["scale"], o["scale"], [o["scale"]], 2, what + " scale")
    assert_within(got["shift"], o["shift"], [o["shift"] + o["mean"] * o["scale"], o["mean"] * o["scale"]], 5,
                  what + " shift")
    assert_within(got["rmean"], o["rmean"], [(1 - MOM) * rmean0, MOM * o["mean"]], 5, what + " rmean")
    assert_within(got["rvar"], o["rvar"], [(1 - MOM) * rvar0, MOM * o["unb"]], 5, what + " rvar")


#   dbeta  = float(s1)                                       1
#   dgamma = float(s2) * rstd                                s2 1, product 1                    = 2
#   A      = gamma * rstd                                    1
#   Cc     = -A * rstd * rstd * float(s2 / M)                A 1, two products 2, s2/M 1, product 1 = 5
#   B      = -A * float(s1 / M) - Cc * mean                  A 1, s1/M 1, product 1, Cc 5, product 1, sub 1 = 10
# e2 (the chain, whose batch mean is no dyadic number): a bound of the fp32 error of s2 itself,
# carried through the expressions: dgamma e2 rstd, Cc e2 |A| rstd^2 / M, B that of Cc times |mean|
def check_bwd_coefs(got, o, what, e2=None, M=1):
    z = torch.zeros_like(o["A"])
    eg = z if e2 is None else e2 * o["rstd"].abs()
    ec = z if e2 is None else e2 * o["A"].abs() * o["rstd"] ** 2 / M
    assert_within(got["dbeta"], o["dbeta"], [o["dbeta"]], 1, what + " dbeta")
    assert_within(got["dgamma"], o["dgamma"], [o["dgamma"]], 2, what + " dgamma", extra=eg)
    assert_within(got["A"], o["A"], [o["A"]], 1, what + " A")
    assert_within(got["Cc"], o["Cc"], [o["Cc"]], 5, what + " Cc", extra=ec)
    assert_within(got["B"], o["B"], [o["t1"], o["t2"]], 10, what + " B", extra=ec * o["mean"].abs())


# ------------------------------------------------------------------ buffers
def vec_in(t, dev):
    """a per-channel fp32 input (any shape, flattened) followed by NaNs"""
    return in_buf(t.reshape(1, -1), t.numel(), F32, dev)


def vec_out(n, dev, init=None):
    full, p = out_buf(1, n, F32, dev)
    if init is not None:
        full[PRE] = init.float().view(torch.int32).to(dev)
    return full, p


def vec_owned(full, n, what):
    assert_guards(full, 1, n, what)
    return owned(full, 1, n, F32).view(-1)


def byte_buf(n, dev):
    full = torch.full((BPRE + n + BPOST,), BSENT, dtype=torch.uint8, device=dev)
    return full, full.data_ptr() + BPRE


def check_bytes(full, ref, what):
    """the n owned bytes equal ref, the guard bytes are untouched"""
    n = ref.numel()
    assert full.numel() == BPRE + n + BPOST, what
    g = torch.cat([full[:BPRE], full[BPRE + n:]])
    assert (g == BSENT).all(), f"{what}: {int((g != BSENT).sum())} mask guard bytes written"
    got = full[BPRE:BPRE + n]
    if not torch.equal(got, ref):
        bad = got != ref
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {n} mask bytes differ, first at {i}: got "
                             f"{int(got[i]):#04x} want {int(ref[i]):#04x}")


def ws_buf(m, C, dev):
    n = m.bn_workspace_floats(C)
    assert n >= 3 * C
    full = torch.full((WPRE + n + WPOST,), SENT32, dtype=torch.int32, device=dev)
    return full, full.data_ptr() + 4 * WPRE, n


def ws_back(full, n, head, name="ws"):
    """what of the workspace travels back: the guards and the first `head` floats"""
    return {name + "_guard": torch.cat([full[:WPRE], full[WPRE + n:]]).cpu(), name: full[WPRE:WPRE + head].cpu()}


def check_ws(res, what, name="ws"):
    assert (res[name + "_guard"] == SENT32).all(), f"{what}: stores outside the workspace"
    return res[name].view(F32)


AMAX_PRE = ("raise", "above0", "below")  # by a case's `apre`


def amax_buf(m, dev, mode):
    """bound_floats() sentinels between guard rows. Block b raises slot b % 16, so slot 0 is hit by
    every launch. 'raise': slots 0; 'above0': slot 0 above every output, the others below every
    block's maximum; 'below': every slot below every block's maximum; 'zero': all sentinels (the
    call must zero what it documents)"""
    n = m.bound_floats()
    assert n == NSLOT * SSTRIDE
    full, p = out_buf(1, n, F32, dev)
    if mode in AMAX_PRE:
        slots = torch.full((NSLOT,), 0.0 if mode == "raise" else BELOW)
        if mode == "above0":
            slots[0] = ABOVE
        full[PRE, ::SSTRIDE] = slots.view(torch.int32).to(dev)
    return full, p


def _bits(v):
    return int(torch.tensor([float(v)], dtype=F32).view(torch.int32)[0])


def _val(bits):
    return torch.tensor([int(bits)], dtype=torch.int32).view(F32)[0]


def check_amax(full, mode, top, what):
    """mode 'raise' / 'above0' / 'below': the call raises the slots (a maximum with what they held,
    never a plain store) and writes nothing else; 'memset': the call zeroed all floats, then raised
    the slots; 'zeroed': the call only zeroed the slot addresses; 'allzero': the call only zeroed
    the whole buffer. top: max |out| (non-negative floats order like their bit patterns); None:
    not known exactly, the caller compares."""
    assert_guards(full, 1, NSLOT * SSTRIDE, what + " amax")
    row = full[PRE]
    slot = row[::SSTRIDE]
    non = row.view(NSLOT, SSTRIDE)[:, 1:]
    if mode in AMAX_PRE + ("zeroed",):
        assert (non == SENT32).all(), f"{what}: amax floats outside the slots written"
    else:
        assert (non == 0).all(), f"{what}: amax floats outside the slots not zeroed"
    if mode in ("zeroed", "allzero"):
        assert (slot == 0).all(), f"{what}: amax slots not zero: {slot.tolist()}"
        return
    assert (slot >= 0).all(), f"{what}: amax slot holds a negative or NaN pattern"
    if top is None:
        return
    tb, lo = _bits(top), _bits(BELOW)
    assert tb > lo or mode not in ("above0", "below"), what
    if mode == "above0":  # block 0 met a larger maximum in its slot: it must still be there
        assert int(slot[0]) == _bits(ABOVE), f"{what}: a larger earlier maximum was replaced"
        slot = slot[1:]
    if mode in ("above0", "below"):  # a slot no block hit keeps its value, a hit one went up
        assert (slot >= lo).all(), f"{what}: an amax slot went down"
    assert (slot <= tb).all(), f"{what}: an amax slot above max |out|"
    if mode == "below":  # block 0 met a smaller maximum in its slot: it must have raised it
        assert int(slot[0]) > lo, f"{what}: slot 0 was not raised above its earlier maximum"
    if mode != "above0":  # (above0: the block that holds the maximum may be one of slot 0's)
        assert int(slot.max()) == tb, f"{what}: amax {_val(slot.max()).item()!r} is not max |out| {float(top)!r}"


# ------------------------------------------------------------------ 1. apply passes, given coefficients
# per-channel coefficient classes (channel % 8), all dyadic. Classes 1 and 2 turn integer data
# into odd integers in [256, 512): exact ties of the bf16 rounding, both signs; class 7 gives
# 10-bit values that round without a tie; class 0 gives zeros and both signs around the ReLU.
FWD_CLASS = ((1, 0), (2, 301), (-2, -301), (.5, .25), (3, -2), (-1, 1), (.25, -.5), (1.5, 300))
BWD_CLASS = ((1, 0, 0), (2, 2, 301), (-2, 2, -301), (.5, .25, .25), (3, -1, -2), (-1, 1, 1), (.25, -.5, -.5),
             (1.5, .5, 300))
C8_M = (1, 63, 64, 65, 255, 256, 257, 511, 513, 1025)
WIDE_C = (24, 72, 64, 512, 2048, 4096, 8192)
WIDE_M = (1, 3, 129)
APPLY_SHAPES = tuple((8, M) for M in C8_M) + tuple((C, M) for C in WIDE_C for M in WIDE_M)
APPLY_OPS = {"apply": [dict(res=r, relu=u) for r in (0, 1) for u in (0, 1)],
             "fwdc": [dict(res=0), dict(res=1)],
             "pair": [dict()],
             "pairb": [dict()],
             "bwdc": [dict(relu=r, dres=d) for r in (0, 1) for d in (0, 1)]}
U0_M = 4096 * 256 + 257  # MPIT_BN_APPLY_U=0: past the 4096-block cap, a ragged second grid-stride trip


def apply_cases(ops=tuple(APPLY_OPS), shapes=APPLY_SHAPES, dts=("bf16", "f32"), variants=None):
    out = []
    for op in ops:
        for v in (variants or APPLY_OPS)[op]:
            for dt in dts:
                for (C, M) in shapes:
                    out.append(dict(op=op, dt=dt, C=C, M=M, apre=1 if M in (3, 63, 257) else 2 if M in (65, 129, 1025) else 0,
                                    **v))
    return out


def _coefs(table, C, rot=0):
    c = torch.arange(C)
    t = torch.tensor(table, dtype=torch.float64)[(c + rot) % 8].t().contiguous()
    t[-1] += 2.0 * ((c // 8) % 5)  # the additive one: an even integer more per 8-channel vector
    return t


def _data(shape, c, g):
    """bf16: integers in [-6, 6]; fp32: the 14-bit `wide` values"""
    return ints(shape, -6, 6, g).double() if c["dt"] == "bf16" else wide(shape, g).double()


def _fma(a, b, cc, what):
    return exact32(a * b + cc, what)


@cached
def gen_apply(c):
    """inputs and fp64 expectations of an apply-pass case; every fmaf and add of the kernel is
    exact in fp32 (asserted), so the expectation is the fp64 value rounded once to the output type"""
    g = _gen(c)
    C, M, op, dt, what = c["C"], c["M"], c["op"], dt_of(c), key(c)
    d, e = {}, {}
    zero = torch.zeros((), dtype=torch.float64)
    if op in ("apply", "fwdc"):
        d["x"], d["coef"] = _data((M, C), c, g), _coefs(FWD_CLASS, C)
        t = _fma(d["x"], d["coef"][0], d["coef"][1], what)
        if c["res"]:
            d["res"] = 2.0 * ints((M, C), -3, 3, g).double() if dt == BF16 else wide((M, C), g).double()
            t = exact32(t + d["res"], what)
        relu = c.get("relu", 1)
        e["mask"] = pack_mask(t > 0)
        e["y"] = (t.clamp(min=0) if relu else t) + 0.0
    elif op == "pair":
        d["x"], d["x2"], d["coef"] = _data((M, C), c, g), _data((M, C), c, g), _coefs(FWD_CLASS, C)
        cc = torch.arange(C)
        d["coef2"] = torch.stack([torch.full((C,), 2.0, dtype=torch.float64), -2.0 * ((cc // 8) % 3)])
        t = exact32(_fma(d["x"], d["coef"][0], d["coef"][1], what) + _fma(d["x2"], d["coef2"][0], d["coef2"][1], what),
                    what)
        e["mask"] = pack_mask(t > 0)
        e["y"] = t.clamp(min=0) + 0.0
    else:
        d["dy"], d["x"], d["coef"] = _data((M, C), c, g), _data((M, C), c, g), _coefs(BWD_CLASS, C)
        dz = d["dy"]
        if c.get("relu", 1):
            d["mask"] = torch.randint(0, 256, (M * C // 8,), generator=g).to(torch.uint8)
            dz = torch.where(unpack_mask(d["mask"], M, C) > 0, dz, zero)
        e["dres"] = dz
        A, Cc, B = d["coef"]
        e["dx"] = _fma(A, dz, _fma(Cc, d["x"], B, what), what) + 0.0
        if op == "pairb":
            d["x2"], d["coef2"] = _data((M, C), c, g), _coefs(BWD_CLASS, C, rot=3)
            A, Cc, B = d["coef2"]
            e["dx2"] = _fma(A, dz, _fma(Cc, d["x2"], B, what), what) + 0.0
    if dt == BF16:  # the rounding to bf16 is put to the test: exact ties among the results
        for name in ("y", "dx", "dx2"):
            if name in e:
                assert bf16_ties(e[name]).any(), f"{what}: no {name} lands on a bf16 tie"
    return d, e


def launch_apply(m, c, dev="cuda"):
    d, _ = gen_apply(c)
    C, M, op, dt = c["C"], c["M"], c["op"], dt_of(c)
    bf = dt == BF16
    s = _stream()
    keep = {k: (in_buf(v, C, dt, dev) if k in ("x", "x2", "res", "dy") else
                torch.cat([v, torch.zeros(64, dtype=torch.uint8)]).to(dev) if k == "mask" else vec_in(v, dev))
            for k, v in d.items()}
    p = {k: v.data_ptr() for k, v in keep.items()}
    out = {}
    mode = AMAX_PRE[c["apre"]]
    assert m.bn_mask_bytes(bf, M, C) == M * C // 8
    if op == "apply":
        out["y"], py = out_buf(M, C, dt, dev)
        m.bn_act_apply(0, s, bf, p["x"], p.get("res", 0), py, M, C, p["coef"], bool(c["relu"]))
    elif op == "fwdc":
        out["y"], py = out_buf(M, C, dt, dev)
        out["mask"], pm = byte_buf(M * C // 8, dev)
        out["amax"], pa = amax_buf(m, dev, mode)
        m.bn_act_fwd(0, s, bf, p["x"], p.get("res", 0), py, M, C, 0, 0, 0, 0, 0, 0, 0, MOM, EPS, True, pm, amax=pa,
                     coef=p["coef"])
    elif op == "pair":
        out["y"], py = out_buf(M, C, dt, dev)
        out["mask"], pm = byte_buf(M * C // 8, dev)
        out["amax"], pa = amax_buf(m, dev, mode)
        m.bn_pair_apply(0, s, p["x"], p["coef"], p["x2"], p["coef2"], py, M, C, pm, f32=not bf, amax=pa)
    elif op == "bwdc":
        out["dx"], pdx = out_buf(M, C, dt, dev)
        pdr = 0
        if c["dres"]:
            out["dres"], pdr = out_buf(M, C, dt, dev)
        out["amax"], pa = amax_buf(m, dev, mode)
        m.bn_act_bwd(0, s, bf, p["dy"], p.get("mask", 0), p["x"], pdx, pdr, M, C, 0, 0, 0, 0, 0, 0, bool(c["relu"]),
                     coef=p["coef"], amax=pa)
    else:
        out["dx"], pdx = out_buf(M, C, dt, dev)
        out["dx2"], pdx2 = out_buf(M, C, dt, dev)
        out["amax"], pa = amax_buf(m, dev, mode)
        out["amax2"], pa2 = amax_buf(m, dev, mode)
        m.bn_pair_bwd_apply(0, s, p["dy"], p["mask"], p["x"], p["coef"], pdx, p["x2"], p["coef2"], pdx2, M, C,
                            f32=not bf, amax1=pa, amax2=pa2)
    torch.cuda.synchronize()
    del keep
    return {k: v.cpu() for k, v in out.items()}


def check_apply(c, res):
    _, e = gen_apply(c)
    C, M, op, dt, what = c["C"], c["M"], c["op"], dt_of(c), key(c)
    mode = AMAX_PRE[c["apre"]]
    for name in ("y", "dx", "dx2", "dres"):
        if name in res:
            assert_guards(res[name], M, C, f"{what} {name}")
            same_bits(owned(res[name], M, C, dt), e[name].float().to(dt), f"{what} {name}")
    if "mask" in res:
        check_bytes(res["mask"], e["mask"], what)
    # the bound is taken from the fp32 values, before a bf16 store rounds them
    for name, of in (("amax", "y" if "y" in e else "dx"), ("amax2", "dx2")):
        if name in res:
            # every 8-channel vector, so every block, holds a value above the pre-filled BELOW
            assert e[of].abs().view(M, C // 8, 8).amax(-1).min().item() > BELOW, what
            check_amax(res[name], mode, e[of].abs().max().float(), f"{what} {name}")


# ------------------------------------------------------------------ 2. stand-alone statistics / reduction
def stat_shapes():
    s = [(C, M) for C in (8, 24, 64, 2048) for M in (1, 2, 7)]
    # rows per block: 8 R, rounded up to R (R = row slots of a block: 256, 32, 1), so M around
    # 8 R (one block / two blocks) and around 16 R (the next seam); then sizes whose row slots
    # take 5 - 7 rows: the 4x / 2x unrolled loops and their tails
    s += [(8, M) for M in (2047, 2048, 2049, 4095, 4096, 4097, 300, 1300)]
    s += [(64, M) for M in (255, 256, 257, 511, 512, 513, 200)]
    s += [(2048, M) for M in (8, 9, 15, 16, 17)]
    s += [(2048, M) for M in (4095, 4096, 4097, 5000)] + [(1024, 8200)]  # the 512-block cap
    s += [(C, M) for C in (24, 72, 200) for M in (7, 333)]                # C % 64 != 0 in the finalize
    s += [(4096, 7), (4096, 129), (8192, 1), (8192, 2), (8192, 7), (8192, 129)]
    return list(dict.fromkeys(s))


def stat_cases(shapes=None, dts=("bf16", "f32")):
    out = []
    for dt in dts:
        for (C, M) in shapes or stat_shapes():
            out.append(dict(op="stat", dir="fwd", dt=dt, C=C, M=M))
            out.append(dict(op="stat", dir="bwd", dt=dt, C=C, M=M, relu=1))
            if M in (1, 7, 257, 1300, 4097, 129):
                out.append(dict(op="stat", dir="bwd", dt=dt, C=C, M=M, relu=0))
    return out


def _affine(C, g):
    return dict(gamma=ints((C,), -16, 16, g).double() / 8, beta=ints((C,), -8, 8, g).double() / 4,
                rmean0=ints((C,), -20, 20, g).double() / 4, rvar0=ints((C,), 1, 40, g).double() / 4)


def _bwd_vectors(c, g):
    """dyadic batch mean and power-of-two rstd: the reduced sums stay exact"""
    C = c["C"]
    return dict(gamma=ints((C,), -16, 16, g).double() / 8, mean=off_of(c) + ints((C,), -8, 8, g).double() / 4,
                rstd=2.0 ** ints((C,), -3, 1, g).double())


def assert_sums_exact(terms, unit, what, window=None):
    """the sum of any subset of `terms` along dim 0 (window: of any `window` consecutive ones), in
    any order, is exact in fp32: every term is a multiple of `unit` and sum |term| stays below
    2^24 units"""
    q = terms / unit
    assert torch.equal(q, q.round()), f"{what}: a term off its granularity"
    if window and window < q.shape[0]:
        cs = torch.cat([torch.zeros_like(q[:1]), q.abs().cumsum(0)])
        top = (cs[window:] - cs[:-window]).max().item()
    else:
        top = q.abs().sum(0).max().item()
    assert top < 2 ** 24, f"{what}: sums reach {top} units, not exact in fp32"


@cached
def gen_stat(c):
    g = _gen(c)
    C, M, what = c["C"], c["M"], key(c)
    d = dict(x=off_of(c) + ints((M, C), -6, 6, g).double())
    if c["dir"] == "fwd":
        d.update(_affine(C, g))
        sh = d["x"] - d["x"][0]  # the kernel's shifted sums (shift = row 0)
        assert_sums_exact(sh, 1.0, what)
        assert_sums_exact(sh * sh, 1.0, what)
        o = bn_forward64(d["x"], d["gamma"], d["beta"], d["rmean0"], d["rvar0"])
    else:
        d.update(_bwd_vectors(c, g))
        d["dy"] = ints((M, C), -6, 6, g).double()
        pos = None
        if c["relu"]:
            d["mask"] = torch.randint(0, 256, (M * C // 8,), generator=g).to(torch.uint8)
            pos = unpack_mask(d["mask"], M, C)
        o = bn_backward64(d["dy"], pos, d["x"], d["gamma"], d["mean"], d["rstd"])
        assert_sums_exact(o["dres"], 1.0, what)
        assert_sums_exact(o["dres"] * (d["x"] - d["mean"]), 0.25, what)
    return d, o


def _launch_fwd_coefs(m, c, d, dev, x, stats=0, nstat=0, amode="zero"):
    """bn_act_fwd with y = 0: coefficients, saved and running statistics"""
    C, M = c["C"], c["M"]
    keep = [vec_in(d["gamma"], dev), vec_in(d["beta"], dev)]
    out = {}
    out["save_mean"], pm = vec_out(C, dev)
    out["save_rstd"], pr = vec_out(C, dev)
    out["rmean"], prm = vec_out(C, dev, d["rmean0"])
    out["rvar"], prv = vec_out(C, dev, d["rvar0"])
    out["amax"], pa = amax_buf(m, dev, amode)
    ws, pw, nws = ws_buf(m, C, dev)
    m.bn_act_fwd(0, _stream(), c["dt"] == "bf16", x.data_ptr(), 0, 0, M, C, keep[0].data_ptr(), keep[1].data_ptr(),
                 prm, prv, pm, pr, pw, MOM, EPS, True, 0, stats=stats, nstat=nstat, amax=pa)
    return out, ws, nws, keep


def _launch_bwd_coefs(m, c, d, dev, x, dy=0, mask=0, part=0, npart=0, amode="zero"):
    """bn_act_bwd with dx = 0: coefficients, dgamma, dbeta"""
    C, M = c["C"], c["M"]
    keep = [vec_in(d["gamma"], dev), vec_in(d["mean"], dev), vec_in(d["rstd"], dev)]
    out = {}
    out["dgamma"], pg = vec_out(C, dev)
    out["dbeta"], pb = vec_out(C, dev)
    out["amax"], pa = amax_buf(m, dev, amode)
    ws, pw, nws = ws_buf(m, C, dev)
    m.bn_act_bwd(0, _stream(), c["dt"] == "bf16", dy, mask, x.data_ptr(), 0, 0, M, C, keep[0].data_ptr(),
                 keep[1].data_ptr(), keep[2].data_ptr(), pg, pb, pw, bool(c.get("relu", 0)), part=part, npart=npart,
                 amax=pa)
    return out, ws, nws, keep


def launch_stat(m, c, dev="cuda"):
    d, _ = gen_stat(c)
    C, dt = c["C"], dt_of(c)
    x = in_buf(d["x"], C, dt, dev)
    if c["dir"] == "fwd":
        out, ws, nws, keep = _launch_fwd_coefs(m, c, d, dev, x)
        head = 2 * C
    else:
        dy = in_buf(d["dy"], C, dt, dev)
        mk = torch.cat([d["mask"], torch.zeros(64, dtype=torch.uint8)]).to(dev) if "mask" in d else None
        out, ws, nws, keep = _launch_bwd_coefs(m, c, d, dev, x, dy.data_ptr(), mk.data_ptr() if mk is not None else 0)
        head = 3 * C
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res.update(ws_back(ws, nws, head))
    del keep
    return res


def _fwd_got(res, C, what):
    w = check_ws(res, what)
    got = {k: vec_owned(res[k], C, f"{what} {k}") for k in ("save_mean", "save_rstd", "rmean", "rvar")}
    got["scale"], got["shift"] = w[:C], w[C:2 * C]
    return got


def _bwd_got(res, C, what, name="ws"):
    w = check_ws(res, what, name)
    got = {k: vec_owned(res[k], C, f"{what} {k}") for k in ("dgamma", "dbeta")}
    got["A"], got["Cc"], got["B"] = w[:C], w[C:2 * C], w[2 * C:3 * C]
    return got


def check_stat(c, res, amode="allzero", gen=None):
    d, o = gen or (gen_stat if c["op"] == "stat" else gen_tile)(c)
    C, what = c["C"], key(c)
    if c["dir"] == "fwd":
        check_fwd_coefs(_fwd_got(res, C, what), o, d["rmean0"], d["rvar0"], what)
    else:
        check_bwd_coefs(_bwd_got(res, C, what), o, what)
    check_amax(res["amax"], amode, 0.0, what)


# ------------------------------------------------------------------ 3. tile partials as input
TILE_NT = (1, 2, 31, 32, 33, 64, 65)
TILE_NT_BIG = (4096, 4100)  # the 128-group cap (C = 8 only: the buffers stay under 20 MB)
TILE_C = (8, 64, 72, 2048)
LAST_ROWS = (1, 64, 127, 128)


def tile_cases(nts=TILE_NT, cs=TILE_C, big=TILE_NT_BIG, dts=("bf16", "f32")):
    out = []
    for dt in dts:
        for i, (C, nt) in enumerate([(C, nt) for C in cs for nt in nts] + [(8, nt) for nt in big]):
            out.append(dict(op="tile", dir="fwd", dt=dt, C=C, nt=nt, last=LAST_ROWS[(i + (dt == "f32")) % 4],
                            M=TILE * (nt - 1) + LAST_ROWS[(i + (dt == "f32")) % 4]))
            out.append(dict(op="tile", dir="bwd", dt=dt, C=C, nt=nt, M=32 * nt + 5))
    return out


def group_rows(nt):
    """most tile rows one level-1 group folds into an fp32 store (bn_act.hip: groups of at least 32
    tile rows, at most 128 groups); the groups themselves are combined in fp64"""
    return max(32, (nt + 127) // 128)


@cached
def gen_tile(c):
    """synthetic partials of 128-row tiles, as the GEMM epilogues write them: forward
    (mean_k, M2_k) of integer data whose last tile holds c['last'] rows, backward integer tile
    sums with more tile rows than ceil(M / 128) (the strided backward-data GEMM's count)"""
    g = _gen(c)
    C, M, nt, what = c["C"], c["M"], c["nt"], key(c)
    if c["dir"] == "bwd":
        d = _bwd_vectors(c, g)
        d["x"] = ints((M, C), -6, 6, g).double()
        d["part"] = torch.stack([ints((nt, C), -500, 500, g).double(), ints((nt, C), -2000, 2000, g).double() / 4], 1)
        assert nt >= (M + TILE - 1) // TILE and (nt < 4 or nt > (M + TILE - 1) // TILE)
        assert_sums_exact(d["part"][:, 0], 1.0, what, group_rows(nt))
        assert_sums_exact(d["part"][:, 1], 0.25, what, group_rows(nt))
        return d, bn_bwd_coefs64(d["part"][:, 0].sum(0), d["part"][:, 1].sum(0), M, d["gamma"], d["mean"], d["rstd"])
    off, n = off_of(c), c["last"]
    x = off + ints((M, C), -6, 6, g).double()
    if n in (64, 127):  # +-v row pairs (and a zero row): the ragged tile's mean is exactly `off`
        v = x[M - n:M - n + n // 2] - off
        x[M - n:] = off + torch.cat([v, -v] + ([torch.zeros(1, C, dtype=torch.float64)] if n % 2 else []))
    d = dict(x=x)
    d.update(_affine(C, g))
    tiles = [x[:M - n].view(nt - 1, TILE, C)] if nt > 1 else []
    mean = torch.cat([t.mean(1) for t in tiles] + [x[M - n:].mean(0, keepdim=True)])
    m2 = torch.cat([((t - t.mean(1, keepdim=True)) ** 2).sum(1) for t in tiles] +
                   [((x[M - n:] - mean[-1]) ** 2).sum(0, keepdim=True)])
    assert torch.equal(mean[:nt - 1] * TILE, (mean[:nt - 1] * TILE).round()), what  # full tiles: integer / 128
    d["part"] = torch.stack([exact32(mean, what), exact32(m2, what)], 1)  # [nt][2][C]
    # the documented combination, fp64, from the fp32 partials
    p = d["part"].float().double()
    nk = torch.full((nt, 1), float(TILE), dtype=torch.float64)
    nk[-1] = n
    dk = p[:, 0] - x[0]
    # every n_k d_k and every M2_k + n_k d_k^2 is an integer (sum and sum of squares of the
    # tile's shifted integers), so the level-1 fp32 store of any group of tile rows is exact
    assert_sums_exact(nk * dk, 1.0, what, group_rows(nt))
    assert_sums_exact(p[:, 1] + nk * dk * dk, 1.0, what, group_rows(nt))
    a, b = (nk * dk).sum(0), (p[:, 1] + nk * dk * dk).sum(0)
    o = bn_coefs64(x[0] + a / M, (b / M - (a / M) ** 2).clamp(min=0), M, d["gamma"], d["beta"], d["rmean0"],
                   d["rvar0"])
    return d, o


def launch_tile(m, c, dev="cuda", sync=True, shared=None, gen=None):
    """shared, gen: device inputs of an earlier launch of the same case and what gen_tile gave
    for it (the ticket-reuse test keeps both); sync=False leaves the results on the device"""
    d, _ = gen or gen_tile(c)
    C, nt, dt = c["C"], c["nt"], dt_of(c)
    if shared is None:
        shared = dict(x=in_buf(d["x"], C, dt, dev), part=in_buf(d["part"].reshape(nt, 2 * C), 2 * C, F32, dev))
    x, part = shared["x"], shared["part"]
    if c["dir"] == "fwd":
        out, ws, nws, keep = _launch_fwd_coefs(m, c, d, dev, x, part.data_ptr(), nt)
        head = 2 * C
    else:
        out, ws, nws, keep = _launch_bwd_coefs(m, c, d, dev, x, part=part.data_ptr(), npart=nt)
        head = 3 * C
    out.update({k: v for k, v in ws_back_dev(ws, nws, head).items()})
    if not sync:
        return out, shared, keep
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def ws_back_dev(full, n, head):
    """ws_back, left on the device (copies queued on the stream of the launch)"""
    return dict(ws_guard=torch.cat([full[:WPRE], full[WPRE + n:]]), ws=full[WPRE:WPRE + head].clone())


def check_tile(c, res, gen=None):
    """the finalize zeroes the slot addresses of amax and nothing else of it"""
    check_stat(c, res, amode="zeroed", gen=gen)


# ------------------------------------------------------------------ 4. the whole chain
CHAIN_SHAPES = ((8, 1), (8, 513), (24, 129), (64, 257), (72, 300), (2048, 4097), (8192, 3))


def chain_cases(shapes=CHAIN_SHAPES, dts=("bf16", "f32")):
    return [dict(op="chain", dt=dt, C=C, M=M) for dt in dts for (C, M) in shapes]


@cached
def gen_chain(c):
    g = _gen(c)
    C, M, what = c["C"], c["M"], key(c)
    d = dict(x=off_of(c) + ints((M, C), -6, 6, g).double(), res=ints((M, C), -3, 3, g).double(),
             dy=ints((M, C), -6, 6, g).double())
    d.update(_affine(C, g))
    sh = d["x"] - d["x"][0]
    assert_sums_exact(sh, 1.0, what)
    assert_sums_exact(sh * sh, 1.0, what)
    assert_sums_exact(d["dy"], 1.0, what)
    return d, bn_forward64(d["x"], d["gamma"], d["beta"], d["rmean0"], d["rvar0"], d["res"])


def launch_chain(m, c, dev="cuda"):
    d, _ = gen_chain(c)
    C, M, dt = c["C"], c["M"], dt_of(c)
    bf = dt == BF16
    s = _stream()
    x, rs, dy = (in_buf(d[k], C, dt, dev) for k in ("x", "res", "dy"))
    ga, be = vec_in(d["gamma"], dev), vec_in(d["beta"], dev)
    out = {}
    out["save_mean"], pm = vec_out(C, dev)
    out["save_rstd"], pr = vec_out(C, dev)
    out["rmean"], prm = vec_out(C, dev, d["rmean0"])
    out["rvar"], prv = vec_out(C, dev, d["rvar0"])
    out["y"], py = out_buf(M, C, dt, dev)
    out["mask"], pk = byte_buf(M * C // 8, dev)
    out["amax"], pa = amax_buf(m, dev, "zero")
    ws, pw, nws = ws_buf(m, C, dev)
    m.bn_act_fwd(0, s, bf, x.data_ptr(), rs.data_ptr(), py, M, C, ga.data_ptr(), be.data_ptr(), prm, prv, pm, pr, pw,
                 MOM, EPS, True, pk, amax=pa)
    out["dx"], pdx = out_buf(M, C, dt, dev)
    out["dres"], pdr = out_buf(M, C, dt, dev)
    out["dgamma"], pg = vec_out(C, dev)
    out["dbeta"], pb = vec_out(C, dev)
    out["amaxb"], pab = amax_buf(m, dev, "zero")
    wsb, pwb, _ = ws_buf(m, C, dev)
    m.bn_act_bwd(0, s, bf, dy.data_ptr(), pk, x.data_ptr(), pdx, pdr, M, C, ga.data_ptr(), pm, pr, pg, pb, pwb, True,
                 amax=pab)
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res.update(ws_back(ws, nws, 2 * C))
    res.update(ws_back(wsb, nws, 3 * C, "wsb"))
    return res


def check_chain(c, res):
    """Forward coefficients as in part 2 (the shifted sums are exact). y, dx against the fp64
    evaluation with the coefficients read back from the workspace: the kernels round twice (y: fmaf,
    + res; dx: two fmaf), so 2 fp32 ulp of the largest term, or for bf16 storage 1 bf16 ulp of
    it. The backward takes the saved mean and rstd the forward wrote (the oracle reads them back), and
    that mean is no dyadic number, so s2 = sum dz (x - mean) rounds in the kernel: each x - mean by
    at most half an ulp of max |x - mean|, each of the additions that fold the M terms (one fmaf per
    row, then at most R per block over at most M / R + 1 blocks: fewer than 2 M + 256 in all) by at
    most half an ulp of S = sum |dz| |x - mean|. That bound of s2's error is carried into the
    part 2 tolerances of dgamma, Cc and B (check_bwd_coefs e2); dbeta and A stay as in part 2."""
    d, o = gen_chain(c)
    C, M, dt, what = c["C"], c["M"], dt_of(c), key(c)
    nr, bits = (0, 8) if dt == BF16 else (1, 24)  # assert_within allows nr + 1 ulp
    got = _fwd_got(res, C, what)
    check_fwd_coefs(got, o, d["rmean0"], d["rvar0"], what)
    sc, sh = got["scale"].double(), got["shift"].double()
    t = d["x"] * sc + sh + d["res"]
    assert_guards(res["y"], M, C, what + " y")
    y = owned(res["y"], M, C, dt)
    assert_within(y, t.clamp(min=0), [d["x"] * sc, sh, d["res"]], nr, what + " y", bits)
    check_bytes(res["mask"], pack_mask(y.double() > 0), what)
    _chain_amax(res["amax"], y, dt, what + " amax")
    # backward
    pos = unpack_mask(res["mask"][BPRE:], M, C)
    dz = d["dy"] * pos
    for name in ("dx", "dres"):
        assert_guards(res[name], M, C, f"{what} {name}")
    same_bits(owned(res["dres"], M, C, dt), (dz + 0.0).float().to(dt), what + " dres")
    gb = _bwd_got(res, C, what, "wsb")
    mu, xm = got["save_mean"].double(), d["x"] - got["save_mean"].double()
    e2 = (2 * M + 256) * 0.5 * ulp((dz.abs() * xm.abs()).sum(0)) + dz.abs().sum(0) * 0.5 * ulp(xm.abs().amax(0))
    ob = bn_bwd_coefs64(dz.sum(0), (dz * xm).sum(0), M, d["gamma"], mu, got["save_rstd"].double())
    check_bwd_coefs(gb, ob, what, e2, M)
    A, Cc, B = gb["A"].double(), gb["Cc"].double(), gb["B"].double()
    dx = owned(res["dx"], M, C, dt)
    assert_within(dx, A * dz + Cc * d["x"] + B, [A * dz, Cc * d["x"], B], nr, what + " dx", bits)
    _chain_amax(res["amaxb"], dx, dt, what + " bwd amax")


def _chain_amax(full, out, dt, what):
    """the stand-alone passes memset the whole buffer, the apply pass raises slots. fp32: the bound
    is exactly the largest stored value. bf16: it is taken before the store rounds, so only its
    rounding can be compared with the largest stored value; check_amax then sees to the zeroed
    floats and the guards alone."""
    top = out.abs().max().float()
    check_amax(full, "memset", top if dt == F32 else None, what)
    if dt == BF16:
        got = _val(full[PRE, ::SSTRIDE].max())
        assert got.to(BF16).item() == top.item(), f"{what}: {got.item()!r} does not round to max |out| {top.item()!r}"


# ------------------------------------------------------------------ dispatch
LAUNCH = {"apply": launch_apply, "fwdc": launch_apply, "pair": launch_apply, "pairb": launch_apply,
          "bwdc": launch_apply, "stat": launch_stat, "tile": launch_tile, "chain": launch_chain}
CHECK = {"apply": check_apply, "fwdc": check_apply, "pair": check_apply, "pairb": check_apply, "bwdc": check_apply,
         "stat": check_stat, "tile": check_tile, "chain": check_chain}
WORKER_VARIANTS = {"apply": [dict(res=1, relu=1)], "fwdc": APPLY_OPS["fwdc"], "pair": [dict()], "pairb": [dict()],
                   "bwdc": [dict(relu=1, dres=1), dict(relu=0, dres=0)]}
WORKER_SHAPES = tuple((8, M) for M in C8_M) + ((24, 129), (64, 129), (512, 3), (2048, 129), (4096, 3))


def worker_cases(env):
    """The reduced list the variant worker runs under the knobs `env` sets: parts 1, 3 and 4."""
    cases = apply_cases(shapes=WORKER_SHAPES, variants=WORKER_VARIANTS)
    cases += tile_cases(nts=(2, 33, 65), cs=(64, 72), big=(4100,)) + tile_cases(nts=(33,), cs=(2048,), big=())
    cases += chain_cases(((8, 513), (64, 257), (512, 129)))
    if env.get("MPIT_BN_APPLY_U") == "0":
        cases += [dict(op="fwdc", dt=dt, C=8, M=U0_M, apre=0, res=0) for dt in ("f32", "bf16")]
    return cases
