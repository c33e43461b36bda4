"""Helpers of tests/test_pool_exact.py and tests/test_act_loss_exact.py: the pooling kernels
(csrc/kernels/pool.hip), relu_bias_bwd / col_sums (act.hip) and softmax_xent (loss.hip) through the
raw bindings against fp64 oracles written from the documented rules.

A case is a dict; ``key(case)`` names and seeds it. ``gen_*`` builds its CPU inputs (in the kernel's
own number format, so what the oracle reads is what the kernel reads) and asserts the exactness
bound the case relies on, the ``*64`` functions evaluate the rules in fp64, ``launch_*`` runs the kernels
and returns whole buffers, guards included, as integer bit patterns (CPU tensors; the few cases
above BIG elements stay on the device, where their oracle runs too: the same torch code),
``check_*`` compares. Inputs carry NaN tail rows, every output sits between sentinel guards, every
workspace has exactly its ``*_ws_floats`` size between sentinels. Nothing of mpit_amd.ops enters
an oracle.

The rules. Max pool forward: the K x K taps in scan order; a tap replaces the best if it is
greater, or a NaN while the best is none; equal values (-0.0 and +0.0 too) keep the first; a
window with nothing above -inf keeps its first in-range tap; the output has the bits of the chosen
input element, the argmax byte is i K + j. Planes output (planes.h): e with bound 2^e in
[2^13, 2^14), h = f16(x 2^e), l = f16(2^11 (x 2^e - h)), slot 0 of the published bound = the max
over the input bound's slots, the other slots +0.0. Max pool backward: dx = the sum of dy over the
windows whose argmax byte names the pixel (+0.0 where none does), with the fused ReLU only of the
windows with ypool > 0 (a subnormal is positive, a NaN is not), db = the column sums of dx as
stored. relu_bias_bwd: dz = dy where y > 0 else +0.0, db = column sums of dz. avgpool_bwd:
dy fp32(1 / HW) in fp32, then rounded to the output type. softmax_xent: loss = log sum exp(x - m)
+ m - x[t] (NaN for t outside [0, C)), d = (softmax - onehot) scale."""
import contextlib
import math
import os
import zlib

import torch

from bn_exact_util import (WPOST, WPRE, assert_sums_exact, assert_within, bf16_ties, byte_buf, cached, check_bytes,
                           exact32, ulp)
from gemm_exact_util import BF16, F32, PRE, SENT32, assert_guards, in_buf, key, out_buf, owned, same_bits, wide

NSLOT, SSTRIDE = 16, 32          # kernels.h kBoundSlots, kBoundStride
BOUND_FLOATS = NSLOT * SSTRIDE   # kBoundFloats
RB_BLOCKS = 8192                 # pool.hip kPoolRbBlocks: block cap of the fused-ReLU backward kernels
RBB_BLOCKS = 1024                # act.hip kMaxBlocks
BIG = 1 << 22                    # elements from which a case is generated compactly and checked on the device
NAN, INF = float("nan"), float("inf")


def dt_of(c):
    return BF16 if c["dt"] == "bf16" else F32


def _idt(dt):
    return torch.int16 if dt == BF16 else torch.int32


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(key(c).encode()))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def sints(shape, lo, hi, g):
    """integers in [lo, hi] as int16 (compact: the large cases hold tens of millions)"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int16)


def tiny(dt):
    """the smallest positive subnormal of the type"""
    return torch.tensor([1], dtype=_idt(dt)).view(dt)[0]


def relu_alphabet(dt):
    """what a ReLU mask must tell apart: -1, -0.0, +0.0, the smallest subnormal, 1, NaN"""
    return torch.stack([torch.tensor(v, dtype=dt) for v in (-1.0, -0.0, 0.0)] + [tiny(dt)] +
                       [torch.tensor(v, dtype=dt) for v in (1.0, NAN)])


def draw(alphabet, shape, g):
    return alphabet[torch.randint(0, alphabet.numel(), tuple(shape), generator=g)]


def big(c):
    return c.get("big", 0) == 1


def guards_intact(full, rows, what, pre=PRE):
    """assert_guards for a buffer whose owned rows are whole (cols == ld), on any device"""
    g = torch.cat([full[:pre], full[pre + rows:]]).cpu()
    assert_guards(g, 0, 0, what, pre=0)


def ws_buf(n, dev):
    """a workspace of exactly n floats between sentinels; (buffer, pointer)"""
    full = torch.full((WPRE + n + WPOST,), SENT32, dtype=torch.int32, device=dev)
    return full, full.data_ptr() + 4 * WPRE


def ws_guards(full, n):
    return torch.cat([full[:WPRE], full[WPRE + n:]]).cpu()


def check_ws_guards(g, what):
    assert g.numel() == WPRE + WPOST and (g == SENT32).all(), f"{what}: stores outside the workspace"


def vec_bits(full, n, what):
    """the n floats a [1, n] output buffer owns, guards checked"""
    assert_guards(full, 1, n, what)
    return owned(full, 1, n, F32).view(-1)


@contextlib.contextmanager
def pool_env(gather):
    """MPIT_POOL_GATHER (read per call by maxpool_bwd) set or unset, restored afterwards"""
    old = os.environ.pop("MPIT_POOL_GATHER", None)
    if gather:
        os.environ["MPIT_POOL_GATHER"] = "1"
    try:
        yield
    finally:
        os.environ.pop("MPIT_POOL_GATHER", None)
        if old is not None:
            os.environ["MPIT_POOL_GATHER"] = old


# ------------------------------------------------------------------ max pool: cases
GEOS = ((3, 2, 1), (2, 2, 0), (3, 3, 0), (3, 1, 1), (5, 3, 2), (2, 1, 1), (1, 1, 0), (15, 4, 7))
# per geometry: 9 x 11 (clipped border windows), K x K (one window), and sizes whose
# (H + 2p - K) % stride != 0; K == stride: every remainder, trailing pixels belong to no window
SIZES = {(3, 2, 1): ((9, 11), (3, 3), (10, 12), (10, 7)),
         (2, 2, 0): ((9, 11), (2, 2), (10, 11), (11, 10)),
         (3, 3, 0): ((9, 11), (3, 3), (10, 9), (11, 10)),
         (3, 1, 1): ((9, 11), (3, 3)),
         (5, 3, 2): ((9, 11), (5, 5), (10, 12)),
         (2, 1, 1): ((9, 11), (2, 2)),
         (1, 1, 0): ((9, 11), (1, 1)),
         (15, 4, 7): ((17, 17), (15, 15), (9, 11), (18, 19))}
POOL_C = (8, 24, 64, 520)
RB_C = (8, 16, 64, 512, 2048)
RB_GEOS = (((3, 2, 1), (9, 11), 0), ((2, 2, 0), (11, 10), 0), ((2, 2, 0), (11, 10), 1), ((3, 3, 0), (10, 11), 0))
DTS = ("bf16", "f32")


def out_hw(c):
    return (c["H"] + 2 * c["p"] - c["K"]) // c["s"] + 1, (c["W"] + 2 * c["p"] - c["K"]) // c["s"] + 1


def partition(c):
    return c["K"] == c["s"] and c["p"] == 0


def pool_cases(geos=GEOS, dts=DTS, cs=POOL_C):
    out, n = [], 0
    for (K, s, p) in geos:
        for (H, W) in SIZES[(K, s, p)]:
            for dt in dts:
                for C in cs:
                    n += 1
                    out.append(dict(op="pool", dt=dt, N=(1, 3)[n % 2] if C != 520 else (3, 1)[n % 2], H=H, W=W, C=C, K=K,
                                    s=s, p=p))
    return out


def special_cases():
    return [dict(op="special", dt=dt, N=2, H=H, W=W, C=8, K=K, s=s, p=p) for dt in DTS
            for (K, s, p), sizes in (((3, 2, 1), ((9, 11), (1, 1), (2, 3))), ((2, 2, 0), ((9, 11), (2, 2), (3, 4))))
            for (H, W) in sizes]


def planes_cases():
    return [dict(op="planes", dt="f32", N=3, H=9, W=11, C=C, K=K, s=s, p=p, bound=b)
            for (K, s, p) in ((3, 2, 1), (2, 2, 0)) for C in (8, 64) for b in (13.0, 100.0)]


def rb_cases(dts=DTS, cs=RB_C):
    return [dict(op="rb", dt=dt, N=2, H=H, W=W, C=C, K=K, s=s, p=p, gather=ga, db=db)
            for dt in dts for C in cs for ((K, s, p), (H, W), ga) in RB_GEOS for db in (0, 1)]


def cap_cases():
    """more threads than the 8192 blocks of the fused-ReLU kernels hold: the gather kernel takes
    N H W C / 8 threads, the per-window kernel N Ho Wo C / 8"""
    return [dict(op="cap", dt="bf16", N=5, H=230, W=230, C=64, K=3, s=2, p=1, gather=0, db=1, big=1),
            dict(op="cap", dt="bf16", N=5, H=461, W=460, C=64, K=2, s=2, p=0, gather=0, db=1, big=1)]


def rb_threads(c):
    Ho, Wo = out_hw(c)
    return c["N"] * (Ho * Wo if partition(c) and not c["gather"] else c["H"] * c["W"]) * c["C"] // 8


# ------------------------------------------------------------------ max pool: oracles (any device)
def _taps(H, W, Ho, Wo, K, s, p, dev):
    """per tap (i, j): its byte, the input rows / columns of the output rows / columns and which
    of them are in range"""
    ho, wo = torch.arange(Ho, device=dev) * s - p, torch.arange(Wo, device=dev) * s - p
    for i in range(K):
        h = ho + i
        vh = (h >= 0) & (h < H)
        for j in range(K):
            w = wo + j
            vw = (w >= 0) & (w < W)
            if vh.any() and vw.any():
                yield i * K + j, h, vh, w, vw


def pool_fwd64(x, K, s, p, count=False):
    """x [N, H, W, C] fp64 -> (best, arg[, how many taps of the window equal its best])"""
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    best = torch.full((N, Ho, Wo, C), -INF, dtype=torch.float64, device=x.device)
    arg = torch.full((N, Ho, Wo, C), -1, dtype=torch.int64, device=x.device)
    for k, h, vh, w, vw in _taps(H, W, Ho, Wo, K, s, p, x.device):
        v = x[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
        valid = (vh[:, None] & vw[None, :])[None, :, :, None]
        take = valid & ((arg < 0) | (v > best) | (v.isnan() & ~best.isnan()))
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    assert (arg >= 0).all()
    if not count:
        return best, arg
    dup = torch.zeros_like(arg)
    for k, h, vh, w, vw in _taps(H, W, Ho, Wo, K, s, p, x.device):
        v = x[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
        dup += ((vh[:, None] & vw[None, :])[None, :, :, None] & (v == best)).long()
    return best, arg, dup


def arg_hw(arg, K, s, p):
    """the input row and column an argmax tap names, per output element"""
    _, Ho, Wo, _ = arg.shape
    h = (torch.arange(Ho, device=arg.device) * s - p)[None, :, None, None] + arg // K
    w = (torch.arange(Wo, device=arg.device) * s - p)[None, None, :, None] + arg % K
    return h, w


def pool_pick(xt, arg, K, s, p):
    """the chosen input elements of the typed input, bit for bit"""
    N, H, W, C = xt.shape
    h, w = arg_hw(arg, K, s, p)
    n = torch.arange(N)[:, None, None, None]
    ch = torch.arange(C)[None, None, None, :]
    return xt.view(_idt(xt.dtype))[n, h, w, ch].view(xt.dtype)


def pool_bwd64(dy, idx, H, W, K, s, p, ypool=None):
    """dy, idx (tap bytes), ypool [N, Ho, Wo, C] -> dx [N, H, W, C] fp64"""
    N, Ho, Wo, C = dy.shape
    zero = torch.zeros((), dtype=torch.float64, device=dy.device)
    g = dy if ypool is None else torch.where(ypool > 0, dy, zero)
    dx = torch.zeros((N, H, W, C), dtype=torch.float64, device=dy.device)
    for k, h, vh, w, vw in _taps(H, W, Ho, Wo, K, s, p, dy.device):
        part = torch.where(idx == k, g, zero)[:, vh][:, :, vw]
        dx[:, h[vh][:, None], w[vw][None, :]] += part  # (one tap: distinct pixels)
    return dx


def stored(v64, dt):
    """fp64 values that are exact in fp32, as the kernel stores them: rounded once to the type"""
    return exact32(v64, "a sum").float().to(dt)


def planes_ref(v64, bound):
    """(h, l, e) of planes.h for fp64 values v and the bound; the decoded value is v itself"""
    e = 14 - math.frexp(bound)[1]
    sx = v64 * 2.0 ** e
    h = sx.half()
    lo = ((sx - h.double()) * 2048.0).half()
    assert torch.equal((h.double() + lo.double() / 2048.0) * 2.0 ** -e, v64), "planes do not carry the value"
    return h, lo, e


# ------------------------------------------------------------------ max pool: generators
SPECIALS = (NAN, INF, -INF, -0.0, 0.0, "tiny", "-tiny", 1.0, -1.0)


def _special_x(c, g):
    """channel e of the 8: 0 NaN, 1 +inf, 2 -inf at the marked pixels of integer data; 3 only zeros
    of both signs; 4 the subnormal at the marked pixels of {-1, -0.0, +0.0}; 5 only -inf (image 0:
    with one NaN); 6 the whole alphabet at random; 7 integers with -inf over the first and last
    three rows and columns (border windows with nothing above -inf). Marked: a corner, a border
    pixel, three neighbours in the middle (one window holds two or three of them), the last pixel;
    the 1 x 1 image is the only in-range tap of its window."""
    N, H, W, dt = c["N"], c["H"], c["W"], dt_of(c)
    x = sints((N, H, W, 8), -3, 3, g).to(dt)
    t = tiny(dt)
    marks = sorted({(0, 0), (0, W // 2), (H // 2, W // 2), (H // 2, max(W // 2 - 1, 0)), (min(H // 2 + 1, H - 1), W // 2),
                    (H - 1, W - 1)})
    mh, mw = torch.tensor([m[0] for m in marks]), torch.tensor([m[1] for m in marks])
    coin = torch.rand((N, H, W), generator=g) < 0.5
    x[..., 3] = torch.where(coin, torch.tensor(-0.0, dtype=dt), torch.tensor(0.0, dtype=dt))
    x[..., 4] = draw(relu_alphabet(dt)[:3], (N, H, W), g)
    x[..., 5] = -INF
    alpha = torch.stack([t if v == "tiny" else -t if v == "-tiny" else torch.tensor(v, dtype=dt) for v in SPECIALS])
    x[..., 6] = draw(alpha, (N, H, W), g)
    x[:, :3, :, 7] = -INF
    x[:, :, :3, 7] = -INF
    x[:, -3:, :, 7] = -INF
    x[:, :, -3:, 7] = -INF
    for e, v in ((0, NAN), (1, INF), (2, -INF), (4, t)):
        x[:, mh, mw, e] = v
    x[0, H // 2, W // 2, 5] = NAN
    return x


def _peaked(shape, dt, g):
    """bf16: integers in [-3, 3]; fp32: the 14-bit `wide` values; a quarter of the elements raised to
    one common peak (ties between peaks, and pixels that several windows select), zeros of both signs"""
    x = sints(shape, -3, 3, g).double() if dt == BF16 else wide(shape, g).double()
    x = torch.where(torch.rand(shape, generator=g) < 0.25, torch.full_like(x, 4.0 if dt == BF16 else 16.0), x)
    x = torch.where((x == 0) & (torch.rand(shape, generator=g) < 0.5), torch.full_like(x, -0.0), x)
    return x.to(dt)


def _pool_dy(shape, g, lim=100):
    """integers, |dy| <= lim: half uniform, half of magnitude in [0.86 lim, lim] with one sign
    per (image, channel), so that the sums over several windows pass 256 and round in bf16"""
    N, _, _, C = shape
    u = sints(shape, -lim, lim, g)
    sign = (sints((N, 1, 1, C), 0, 1, g) * 2 - 1)
    b = sints(shape, int(0.86 * lim), lim, g) * sign
    return torch.where(torch.rand(shape, generator=g) < 0.5, u, b).double()


def _tie_dy(dy, arg, H, W, K, s, p, g):
    """at half of the pixels that three or more windows select, the gradients of those windows become
    +-(100, 100, 57, 0, ...) in tap order: the sum is +-257, half way between two bf16 numbers"""
    dy = dy.clone()
    N, Ho, Wo, C = dy.shape
    cnt = pool_bwd64(torch.ones_like(dy), arg, H, W, K, s, p)
    pick = (cnt >= 3) & (torch.rand(cnt.shape, generator=g) < 0.5)
    sign = torch.where(torch.rand(cnt.shape, generator=g) < 0.5, -1.0, 1.0).double()
    run = torch.zeros_like(cnt)
    vals = torch.tensor([100.0, 100.0, 57.0], dtype=torch.float64)
    for k, h, vh, w, vw in _taps(H, W, Ho, Wo, K, s, p, dy.device):
        hv, wv = h[vh][:, None], w[vw][None, :]
        ho, wo = vh.nonzero().view(-1)[:, None], vw.nonzero().view(-1)[None, :]
        sel = (arg == k)[:, ho, wo]
        r = run[:, hv, wv].long()
        v = torch.where(r < 3, vals[r.clamp(max=2)], torch.zeros_like(cnt[:, hv, wv])) * sign[:, hv, wv]
        dy[:, ho, wo] = torch.where(sel & pick[:, hv, wv], v, dy[:, ho, wo])
        run[:, hv, wv] += sel.double()
    return dy


def expects_ties(c):
    """overlapped windows on an image of several windows: a pixel collects 3 or more gradients"""
    return c["dt"] == "bf16" and c["K"] >= 2 * c["s"] - 1 and c["K"] > c["s"] and min(c["H"], c["W"]) >= 9 \
        and c["op"] == "pool"


@cached
def gen_pool(c):
    """x, dy (and ypool) of a pool / special / planes / rb case, in the kernel's type, with the
    oracle's forward (arg = the tap per output element) and the plain and fused backward"""
    g = _gen(c)
    N, H, W, C, K, s, p, dt, what = c["N"], c["H"], c["W"], c["C"], c["K"], c["s"], c["p"], dt_of(c), key(c)
    Ho, Wo = out_hw(c)
    d = {}
    if c["op"] == "special":
        d["x"] = _special_x(c, g)
    elif c["op"] == "planes":
        d["x"] = wide((N, H, W, C), g)
    else:
        d["x"] = _peaked((N, H, W, C), dt, g)
        # every fourth channel: one value above the peaks at the last tap of window (0, 0), the
        # largest byte, K K - 1
        d["x"][:, K - 1 - p, K - 1 - p, ::4] = 32.0
    best, arg, dup = pool_fwd64(d["x"].double(), K, s, p, count=True)
    if c["op"] != "special" and K > 1 and min(H, W) >= 9:
        assert (dup > 1).any(), f"{what}: no window has a tie for its maximum"
    o = dict(arg=arg, idx=arg.to(torch.uint8), y=pool_pick(d["x"], arg, K, s, p))
    assert int(arg.max()) < K * K and torch.equal(o["y"].double().nan_to_num(7e77), best.nan_to_num(7e77)), what
    if c["op"] == "planes":
        return d, o
    assert c["op"] == "special" or (arg[:, 0, 0, ::4] == K * K - 1).all(), what
    d["dy"] = _pool_dy((N, Ho, Wo, C), g)
    if expects_ties(c):
        d["dy"] = _tie_dy(d["dy"], arg, H, W, K, s, p, g)
    d["dy"] = d["dy"].to(dt)
    yp = None
    if c["op"] == "rb":
        d["ypool"] = draw(relu_alphabet(dt), (N, Ho, Wo, C), g)
        yp = d["ypool"].double()
    dx = pool_bwd64(d["dy"].double(), arg, H, W, K, s, p, yp)
    o["dx"] = stored(dx, dt)
    if expects_ties(c):
        assert bf16_ties(dx).any(), f"{what}: no dx sum lands on a bf16 tie"
    if c["op"] == "rb":
        o["db"] = _db_of(o["dx"], what)
    return d, o


def _db_of(dx_stored, what):
    """column sums of the stored values: integers, below 2^24 in all, so exact in any order"""
    v = dx_stored.double().reshape(-1, dx_stored.shape[-1])
    assert_sums_exact(v, 1.0, what)
    return v.sum(0).float()


@cached
def gen_cap(c):
    """Synthetic argmax bytes (every one a legal in-range tap: the first row / column of windows of
    the padded geometry never names its padding), dy in [-4, 4], the ReLU alphabet as ypool."""
    g = _gen(c)
    N, C, K, dt = c["N"], c["C"], c["K"], dt_of(c)
    Ho, Wo = out_hw(c)
    i, j = sints((N, Ho, Wo, C), 0, K - 1, g), sints((N, Ho, Wo, C), 0, K - 1, g)
    if c["p"]:
        assert c["p"] == 1 and (Ho - 1) * c["s"] - 1 + K <= c["H"] and (Wo - 1) * c["s"] - 1 + K <= c["W"]
        i[:, 0] = i[:, 0].clamp(min=1)
        j[:, :, 0] = j[:, :, 0].clamp(min=1)
    d = dict(idx=(i * K + j).to(torch.uint8), dy=sints((N, Ho, Wo, C), -4, 4, g).to(dt),
             ypool=draw(relu_alphabet(dt), (N, Ho, Wo, C), g))
    # at most ceil(K / s)^2 windows reach a pixel: small integers, stored without rounding, and
    # the column sums of their magnitudes stay below 2^24
    assert 4 * N * Ho * Wo * 4 < 2 ** 24 and rb_threads(c) > RB_BLOCKS * 256, key(c)
    return d


# ------------------------------------------------------------------ max pool: launches and checks
def _geo(c):
    return c["N"], c["H"], c["W"], c["C"], c["K"], c["s"], c["p"]


def _idx_in(idx, dev):
    """argmax bytes as an input: followed by bytes no tap has"""
    return torch.cat([idx.reshape(-1), torch.full((64,), 0xFF, dtype=torch.uint8)]).to(dev)


def bwd_variants(c):
    """(name, MPIT_POOL_GATHER) of the backward kernels a geometry has"""
    return (("part", 0), ("gather", 1)) if partition(c) else (("gather", 0),)


def launch_pool(m, c, dev="cuda", own=False):
    """forward, then the backward of every kernel the geometry has, fed the oracle's argmax bytes
    (own: once more fed the bytes the forward wrote)"""
    d, o = gen_pool(c)
    N, H, W, C, K, s, p = _geo(c)
    Ho, Wo = out_hw(c)
    dt, f32, st = dt_of(c), c["dt"] == "f32", _stream()
    x = in_buf(d["x"].reshape(-1, C), C, dt, dev)
    res = {}
    res["y"], py = out_buf(N * Ho * Wo, C, dt, dev)
    res["idx"], pi = byte_buf(N * Ho * Wo * C, dev)
    m.maxpool_fwd(0, st, N, H, W, C, K, s, p, x.data_ptr(), py, pi, f32=f32)
    dy, idx = in_buf(d["dy"].reshape(-1, C), C, dt, dev), _idx_in(o["idx"], dev)
    for name, ga in bwd_variants(c) + ((("own", 0),) if own else ()):
        res["dx_" + name], pdx = out_buf(N * H * W, C, dt, dev)
        with pool_env(ga):
            m.maxpool_bwd(0, st, N, H, W, C, K, s, p, dy.data_ptr(), pi if name == "own" else idx.data_ptr(), pdx, f32=f32)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def check_pool(c, res):
    _, o = gen_pool(c)
    N, H, W, C, _, _, _ = _geo(c)
    Ho, Wo = out_hw(c)
    dt, what = dt_of(c), key(c)
    assert_guards(res["y"], N * Ho * Wo, C, what + " y")
    same_bits(owned(res["y"], N * Ho * Wo, C, dt), o["y"].reshape(-1, C), what + " y")
    check_bytes(res["idx"], o["idx"].reshape(-1), what + " argmax")
    for name in ("part", "gather", "own"):
        if "dx_" + name in res:
            assert_guards(res["dx_" + name], N * H * W, C, f"{what} dx {name}")
            same_bits(owned(res["dx_" + name], N * H * W, C, dt), o["dx"].reshape(-1, C), f"{what} dx {name}")


def bound_in(bound, dev):
    """the input's slotted bound: the maximum in slot 5, smaller values, zero and NaN floats between"""
    b = torch.full((BOUND_FLOATS + 32,), NAN)
    b[:BOUND_FLOATS:SSTRIDE] = torch.tensor([0.0 if k == 0 else bound if k == 5 else bound / (k + 2) for k in range(NSLOT)])
    return b.to(dev)


def launch_planes(m, c, dev="cuda"):
    d, _ = gen_pool(c)
    N, H, W, C, K, s, p = _geo(c)
    Ho, Wo = out_hw(c)
    x, ib = in_buf(d["x"].reshape(-1, C), C, F32, dev), bound_in(c["bound"], dev)
    res = {}
    res["y"], py = out_buf(N * Ho * Wo, C, F32, dev)
    res["idx"], pi = byte_buf(N * Ho * Wo * C, dev)
    res["obound"], po = out_buf(1, BOUND_FLOATS, F32, dev)
    assert m.bound_floats() == BOUND_FLOATS
    m.maxpool_fwd(0, _stream(), N, H, W, C, K, s, p, x.data_ptr(), py, pi, f32=True, ibound=ib.data_ptr(), obound=po)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def check_planes(c, res):
    _, o = gen_pool(c)
    N, _, _, C, _, _, _ = _geo(c)
    Ho, Wo = out_hw(c)
    what, rows = key(c), N * Ho * Wo
    h, lo, e = planes_ref(o["y"].double().reshape(-1), c["bound"])
    assert_guards(res["y"], rows, C, what + " y")
    got = res["y"][PRE:PRE + rows].contiguous().view(torch.int16).reshape(-1)  # h plane, then l plane
    for name, plane, ref in (("h", got[:rows * C], h), ("l", got[rows * C:], lo)):
        if not torch.equal(plane, ref.view(torch.int16)):
            bad = plane != ref.view(torch.int16)
            raise AssertionError(f"{what}: {int(bad.sum())} {name} halves differ, first at {int(bad.nonzero()[0])}")
    dec = (got[:rows * C].view(torch.float16).double() + got[rows * C:].view(torch.float16).double() / 2048.0) * 2.0 ** -e
    assert torch.equal(dec, o["y"].double().reshape(-1)), f"{what}: decoded planes are not the chosen inputs"
    check_bytes(res["idx"], o["idx"].reshape(-1), what + " argmax")
    assert_guards(res["obound"], 1, BOUND_FLOATS, what + " obound")
    row = res["obound"][PRE]
    slot = torch.zeros(NSLOT, dtype=F32)
    slot[0] = c["bound"]
    assert torch.equal(row[::SSTRIDE], slot.view(torch.int32)), \
        f"{what}: published bound slots {row[::SSTRIDE].view(F32).tolist()}"
    assert (row.view(NSLOT, SSTRIDE)[:, 1:] == SENT32).all(), f"{what}: bound floats outside the slots written"


def _launch_bwd_rb(m, c, d, idx, dev):
    """maxpool_bwd with ypool (and db) on device inputs; the results stay on the device"""
    N, H, W, C, K, s, p = _geo(c)
    dt, f32 = dt_of(c), c["dt"] == "f32"
    dy, yp = in_buf(d["dy"].reshape(-1, C), C, dt, dev), in_buf(d["ypool"].reshape(-1, C), C, dt, dev)
    ix = _idx_in(idx, dev)
    nws = m.maxpool_bwd_ws_floats(C)
    assert nws == RB_BLOCKS * C + m.col_sums_ws_floats(C)
    res = {}
    res["dx"], pdx = out_buf(N * H * W, C, dt, dev)
    ws, pw = ws_buf(nws, dev)
    pdb = 0
    if c["db"]:
        res["db"], pdb = out_buf(1, C, F32, dev)
    with pool_env(c["gather"]):
        m.maxpool_bwd(0, _stream(), N, H, W, C, K, s, p, dy.data_ptr(), ix.data_ptr(), pdx, f32=f32, ypool=yp.data_ptr(),
                      db=pdb, ws=pw)
    torch.cuda.synchronize()
    res["ws_guard"] = ws_guards(ws, nws)
    del dy, yp, ix
    return res


def launch_rb(m, c, dev="cuda"):
    d, o = gen_pool(c)
    return {k: v.cpu() for k, v in _launch_bwd_rb(m, c, d, o["idx"], dev).items()}


def check_rb(c, res):
    _, o = gen_pool(c)
    N, H, W, C, _, _, _ = _geo(c)
    dt, what = dt_of(c), key(c)
    assert_guards(res["dx"], N * H * W, C, what + " dx")
    same_bits(owned(res["dx"], N * H * W, C, dt), o["dx"].reshape(-1, C), what + " dx")
    check_ws_guards(res["ws_guard"], what)
    assert ("db" in res) == bool(c["db"])
    if c["db"]:
        same_bits(vec_bits(res["db"], C, what + " db"), o["db"], what + " db")


def run_cap(m, c, dev="cuda"):
    """launch and check on the device: the fp64 oracle of these sizes takes the CPU too long"""
    d = gen_cap(c)
    N, H, W, C, K, s, p = _geo(c)
    dt, what = dt_of(c), key(c)
    res = _launch_bwd_rb(m, c, d, d["idx"], dev)
    dx = pool_bwd64(d["dy"].to(dev).double(), d["idx"].to(dev), H, W, K, s, p, d["ypool"].to(dev).double())
    ref = stored(dx, dt)
    del dx
    guards_intact(res["dx"], N * H * W, what + " dx")
    same_bits(res["dx"][PRE:PRE + N * H * W].view(dt), ref.reshape(-1, C), what + " dx")
    check_ws_guards(res["ws_guard"], what)
    v = ref.double().reshape(-1, C)
    assert v.abs().sum(0).max().item() < 2 ** 24 and torch.equal(v, v.round()), what
    same_bits(vec_bits(res["db"].cpu(), C, what + " db"), v.sum(0).float().cpu(), what + " db")


# ------------------------------------------------------------------ avgpool_bwd
def avg_cases():
    return [dict(op="avg", dt=dt, N=N, HW=HW, C=C) for dt in DTS for N in (1, 3) for HW in (1, 4, 49, 64)
            for C in (8, 72, 256)]


@cached
def gen_avg(c):
    """dy with full mantissas (a power-of-two HW divides exactly whatever they hold)"""
    return torch.randn((c["N"], c["C"]), generator=_gen(c)).mul(3).to(dt_of(c))


def launch_avg(m, c, dev="cuda"):
    N, HW, C, dt = c["N"], c["HW"], c["C"], dt_of(c)
    dy = in_buf(gen_avg(c), C, dt, dev)
    full, pdx = out_buf(N * HW, C, dt, dev)
    m.avgpool_bwd(0, _stream(), N, HW, C, dy.data_ptr(), pdx, f32=c["dt"] == "f32")
    torch.cuda.synchronize()
    return {"dx": full.cpu()}


def check_avg(c, res):
    N, HW, C, dt, what = c["N"], c["HW"], c["C"], dt_of(c), key(c)
    dy = gen_avg(c)
    assert_guards(res["dx"], N * HW, C, what)
    got = owned(res["dx"], N * HW, C, dt).view(N, HW, C)
    ref = (dy.double() / HW)[:, None, :].expand(N, HW, C)
    if HW & (HW - 1) == 0:
        same_bits(got, ref.float().to(dt).contiguous(), what)
        return
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(HW), dtype=F32)
    two = (dy.float() * inv)[:, None, :].expand(N, HW, C).contiguous()
    if dt == BF16:
        same_bits(got, two.to(BF16), what)
    else:  # 1 / HW rounds, the product rounds
        assert_within(got, ref, [ref], 2, what)


# ------------------------------------------------------------------ relu_bias_bwd
RBB_C = (8, 24, 64, 1024, 2040, 2400, 8192)


def rbb_rows(C):
    """R of relu_bias_bwd: row slots of a block (256 threads rounded down to whole rows of C / 8)"""
    G = C // 8
    return (G if G >= 256 else 256 // G * G) // G


def rbb_cases(dts=DTS):
    out = []
    for dt in dts:
        for C in RBB_C:
            R = rbb_rows(C)
            for M in sorted({1, 15, 16 * R - 1, 16 * R, 16 * R + 1, 5000}):
                out.append(dict(op="rbb", dt=dt, C=C, M=M, db=1, big=int(M * C >= BIG)))
                if M in (15, 16 * R + 1):
                    out.append(dict(op="rbb", dt=dt, C=C, M=M, db=0, big=int(M * C >= BIG)))
        # past the 1024-block cap: more than 1024 blocks' worth of 16 R rows
        out.append(dict(op="rbb", dt=dt, C=8, M=RBB_BLOCKS * 16 * rbb_rows(8) + 4097, db=1, big=1))
    return out


@cached
def gen_rbb(c):
    g = _gen(c)
    M, C, dt = c["M"], c["C"], dt_of(c)
    lim = 100 if M * 100 < 2 ** 24 else 3
    assert M * lim < 2 ** 24, key(c)  # integer columns: |sum| < 2^24 in any order
    dy = sints((M, C), -lim, lim, g).to(dt)
    dy = torch.where((dy == 0) & (torch.rand((M, C), generator=g) < 0.5), torch.tensor(-0.0, dtype=dt), dy)
    return dict(dy=dy, y=draw(relu_alphabet(dt), (M, C), g))


def launch_rbb(m, c, dev="cuda"):
    d = gen_rbb(c)
    M, C, dt = c["M"], c["C"], dt_of(c)
    dy, y = in_buf(d["dy"], C, dt, dev), in_buf(d["y"], C, dt, dev)
    res = {}
    res["dz"], pz = out_buf(M, C, dt, dev)
    pdb = pw = 0
    if c["db"]:
        nws = m.relu_bias_bwd_ws_floats(C)
        res["db"], pdb = out_buf(1, C, F32, dev)
        ws, pw = ws_buf(nws, dev)
    m.relu_bias_bwd(0, _stream(), M, C, dy.data_ptr(), y.data_ptr(), pz, pdb, pw, f32=c["dt"] == "f32")
    torch.cuda.synchronize()
    if c["db"]:
        res["ws_guard"] = ws_guards(ws, nws)
    return res if big(c) else {k: v.cpu() for k, v in res.items()}


def check_rbb(c, res):
    d = gen_rbb(c)
    M, C, dt, what = c["M"], c["C"], dt_of(c), key(c)
    dev = res["dz"].device
    dy, y = d["dy"].to(dev), d["y"].to(dev)
    dz = torch.where(y.double() > 0, dy, torch.zeros((), dtype=dt, device=dev))
    guards_intact(res["dz"], M, what + " dz")
    same_bits(res["dz"][PRE:PRE + M].view(dt), dz, what + " dz")
    assert ("db" in res) == bool(c["db"])
    if c["db"]:
        check_ws_guards(res["ws_guard"], what)
        same_bits(vec_bits(res["db"].cpu(), C, what + " db"), dz.double().sum(0).float().cpu(), what + " db")


# ------------------------------------------------------------------ col_sums
CS_NB = (1, 15, 16, 17, 64, 65, 66, 1000, 1024, 8192)
CS_C = (8, 64, 72, 1000)


def cs_cases():
    return [dict(op="cs", nb=nb, C=C, ld=ld, mid=int(nb > 64 or (nb + C) % 2))
            for nb in CS_NB for C in CS_C for ld in sorted({C, 2 * C, C + 8})]


@cached
def gen_cs(c):
    assert c["nb"] * 100 < 2 ** 24
    return sints((c["nb"], c["C"]), -100, 100, _gen(c)).float()


def launch_cs(m, c, dev="cuda"):
    nb, C, ld = c["nb"], c["C"], c["ld"]
    part = in_buf(gen_cs(c), ld, F32, dev)
    res, pm = {}, 0
    res["out"], po = out_buf(1, C, F32, dev)
    if c["mid"]:
        nws = m.col_sums_ws_floats(C)
        ws, pm = ws_buf(nws, dev)
    m.col_sums(0, _stream(), part.data_ptr(), nb, ld, C, po, pm)
    torch.cuda.synchronize()
    if c["mid"]:
        res["ws_guard"] = ws_guards(ws, nws)
    return {k: v.cpu() for k, v in res.items()}


def check_cs(c, res):
    what = key(c)
    same_bits(vec_bits(res["out"], c["C"], what), gen_cs(c).double().sum(0).float(), what)
    if c["mid"]:
        check_ws_guards(res["ws_guard"], what)


# ------------------------------------------------------------------ softmax_xent
XE_C = (1, 2, 10, 255, 256, 257, 513, 1000, 4097)
XE_ROWS = (1, 3, 300)
XE_SCALE = (1.0, 2.0 ** -8)


def xent_cases(kind, dts=DTS):
    out, n = [], 0
    for dt in dts:
        for C in XE_C:
            for ldx in (C, (C + 63) // 64 * 64):
                for rows in XE_ROWS:
                    n += 1
                    out.append(dict(op="xent", kind=kind, dt=dt, C=C, ldx=ldx, rows=rows, scale=XE_SCALE[n % 2]))
    return out


def _targets(rows, C, g):
    """random classes; of every 7 rows one has the target -1 and one the target C"""
    t = torch.randint(0, C, (rows,), generator=g)
    r = torch.arange(rows)
    return torch.where(r % 7 == 5, torch.full_like(t, -1), torch.where(r % 7 == 6, torch.full_like(t, C), t))


@cached
def gen_xent(c):
    """structural: m at j columns (j a power of two; the block of maxima starts at column 0, ends at
    the last column, or starts past the first 256-column sweep, by row), m - 200 elsewhere, m a small
    integer; every third row's target is a maximum. numeric: 4 randn, every fifth row spans +-30."""
    g = _gen(c)
    rows, C, dt = c["rows"], c["C"], dt_of(c)
    t = _targets(rows, C, g)
    if c["kind"] == "num":
        x = torch.randn((rows, C), generator=g) * 4
        for r in range(0, rows, 5):
            x[r] = (torch.linspace(-30, 30, C) if C > 1 else torch.tensor([30.0]))[torch.randperm(C, generator=g)]
        return dict(x=x.to(dt), t=t)
    m = sints((rows,), -3, 3, g).double()
    x = (m - 200.0)[:, None].repeat(1, C)
    j = torch.zeros(rows, dtype=torch.int64)
    for r in range(rows):
        jr = min(1 << ((r // 3) % 4), 1 << (C.bit_length() - 1))
        a = (0, C - jr, 256 if C >= 256 + jr else (C - jr) // 2)[r % 3]
        x[r, a:a + jr] = m[r]
        j[r] = jr
        if r % 3 == 0 and 0 <= t[r] < C:
            t[r] = a + jr - 1
    assert torch.equal(x.to(dt).double(), x)
    return dict(x=x.to(dt), t=t, m=m, j=j)


def xent64(x, t):
    """fp64: per-row loss (NaN for a target outside [0, C)) and softmax - onehot"""
    rows, C = x.shape
    m = x.amax(1, keepdim=True)
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    ok = (t >= 0) & (t < C)
    xt = x.gather(1, t.clamp(0, C - 1)[:, None])[:, 0]
    loss = torch.where(ok, torch.log(s[:, 0]) + m[:, 0] - xt, torch.full_like(xt, NAN))
    onehot = (torch.arange(C, device=x.device)[None, :] == t[:, None]).double()
    return loss, e / s - onehot


def launch_xent(m, c, dev="cuda", d=None):
    d = d or gen_xent(c)
    rows, C, ldx, dt = c["rows"], c["C"], c["ldx"], dt_of(c)
    x = in_buf(d["x"], ldx, dt, dev)
    t = torch.cat([d["t"], torch.full((8,), -(2 ** 40))]).to(dev)
    res = {}
    res["loss"], pl = out_buf(1, rows, F32, dev)
    res["d"], pd = out_buf(rows, C, F32, dev)
    m.softmax_xent(0, _stream(), rows, C, x.data_ptr(), ldx, c["dt"] == "bf16", t.data_ptr(), c["scale"], pl, pd)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def xent_got(c, res):
    what = key(c)
    assert_guards(res["d"], c["rows"], c["C"], what + " d")
    return vec_bits(res["loss"], c["rows"], what + " loss"), owned(res["d"], c["rows"], c["C"], F32)


def check_xent_struct(c, res):
    """Bitwise: exp is exactly 1 or 0, s = j, so d = (1 / j or 0, minus the one-hot) scale with j and
    scale powers of two; with j = 1 the loss is m - x[t] exactly. Returns the rows with j > 1 (their
    loss holds logf(j): compared like the numeric cases)."""
    d = gen_xent(c)
    rows, C, what = c["rows"], c["C"], key(c)
    loss, dd = xent_got(c, res)
    x, t = d["x"].double(), d["t"]
    ok = (t >= 0) & (t < C)
    onehot = (torch.arange(C)[None, :] == t[:, None]).double()
    ref = ((x == d["m"][:, None]).double() / d["j"][:, None] - onehot) * c["scale"] + 0.0
    same_bits(dd, exact32(ref, what).float(), what + " d")
    assert torch.equal(loss.isnan(), ~ok), f"{what}: the NaN losses are not those of the targets outside [0, C)"
    one = ok & (d["j"] == 1)
    xt = x.gather(1, t.clamp(0, C - 1)[:, None])[:, 0]
    same_bits(loss[one], (d["m"] - xt)[one].float() + 0.0, what + " loss")
    assert set((d["m"] - xt)[one].tolist()) <= {0.0, 200.0}
    return ok & (d["j"] > 1)


def fp32_class(got, ref, lib, top, what):
    """the kernel's max error against fp64 is at most twice the library's on the same tensor, plus
    one fp32 ulp of the largest term; both errors are printed"""
    ek, el = (got.double() - ref).abs().max().item(), (lib.double() - ref).abs().max().item()
    floor = ulp(torch.tensor(float(top), dtype=torch.float64)).item()
    print(f"{what}: kernel {ek:.3e} library {el:.3e} ulp {floor:.3e}")
    assert ek <= 2 * el + floor, f"{what}: kernel error {ek:.3e} above 2 x {el:.3e} + {floor:.3e}"


def check_xent_lib(c, res, rows_sel=None, dev="cuda"):
    """loss and d / scale against fp64, measured against PyTorch's fp32 log_softmax / nll_loss and
    softmax gradient of the same logits on the same device (tests/test_fp32_path.py's fp32 class)"""
    import torch.nn.functional as F

    d = gen_xent(c)
    C, what = c["C"], key(c)
    loss, dd = xent_got(c, res)
    t = d["t"]
    ok = (t >= 0) & (t < C) if rows_sel is None else rows_sel
    if not ok.any():
        return
    x, t = d["x"][ok], t[ok]
    l64, d64 = xent64(x.double(), t)
    xg = x.float().to(dev).requires_grad_(True)
    ll = F.nll_loss(F.log_softmax(xg, dim=1), t.to(dev), reduction="none")
    ll.sum().backward()
    xt = x.double().gather(1, t[:, None])[:, 0]
    top = torch.stack([l64 + xt - x.double().amax(1), x.double().amax(1), xt]).abs().max()
    fp32_class(loss[ok], l64, ll.detach().cpu(), top, what + " loss")
    if rows_sel is None:
        fp32_class(dd[ok] / c["scale"], d64, xg.grad.cpu(), 1.0, what + " d / scale")
        # the rows with a target outside [0, C): NaN loss, the softmax with no one-hot subtracted
        out = ~ok
        assert loss[out].isnan().all() and not loss[ok].isnan().any(), what
        if out.any():
            p64 = torch.softmax(d["x"][out].double(), 1)
            lib = torch.softmax(d["x"][out].float().to(dev), 1).cpu()
            fp32_class(dd[out] / c["scale"], p64, lib, 1.0, what + " d / scale, target outside")


LAUNCH = {"pool": launch_pool, "special": launch_pool, "planes": launch_planes, "rb": launch_rb, "avg": launch_avg,
          "rbb": launch_rbb, "cs": launch_cs}
CHECK = {"pool": check_pool, "special": check_pool, "planes": check_planes, "rb": check_rb, "avg": check_avg,
         "rbb": check_rbb, "cs": check_cs}


def run_cases(m, cases, launch=None, check=None):
    """Launch and check every case; mismatches are collected so one run names them all (anything
    but a failed comparison, a HIP error for instance, ends the run at once)."""
    bad = []
    for c in cases:
        res = (launch or LAUNCH[c["op"]])(m, c)
        try:
            (check or CHECK[c["op"]])(c, res)
        except AssertionError as e:
            bad.append(str(e)[:300])
    print(f"{len(cases)} cases compared, {len(bad)} failed")
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad[:12])
