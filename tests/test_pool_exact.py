"""Exact oracles for the pooling kernels (csrc/kernels/pool.hip) at their edges.

A max pool moves values and sums gradients, so every output bit is pinned: the forward's output has
the bits of the input element the documented scan-order rule chooses and its argmax byte names that
tap (ties, -0.0 against +0.0, NaN, +-inf, subnormals, border windows with nothing above -inf); the
backward over integer gradients is bitwise the fp64 sum, rounded once to nearest even for bf16 (the
generators assert that ties occur); the fused ReLU takes the windows with ypool > 0 and its bias
gradient is the exact column sum of what was stored. The backward is fed the oracle's argmax bytes,
so a forward error cannot cancel (one test feeds it the forward's own). Inputs end in NaN rows,
outputs, argmax bytes, the published bound and the workspace sit between sentinels. All calls go
through the raw bindings of mpit_amd._ext.native(); helpers in tests/pool_exact_util.py.

Measured on an MI355X machine: the GPU tests of this file take 4 s together; the slowest are
test_maxpool_exact[k15s4p7-bf16] (1.2 s: 225 taps per window in the oracle), the gather case past the
block cap (0.6 s, 17 M elements, oracle on the device) and the per-window one (0.3 s, 68 M elements);
every other test stays below 0.4 s."""
import pytest
import torch
import torch.nn.functional as F

import pool_exact_util as U
from bn_exact_util import BPRE, bf16_ties, byte_buf
from gemm_exact_util import BF16, F32, PRE, key, out_buf, same_bits

gpu = pytest.mark.gpu


def _m():
    from mpit_amd._ext import native

    return native()


def _run(cases, launch=None, check=None):
    U.run_cases(_m(), cases, launch, check)


# ------------------------------------------------------------------ CPU: the net itself
@pytest.mark.parametrize("geo", U.GEOS, ids=lambda g: "k%ds%dp%d" % g)
def test_oracle_matches_fp64_max_pool2d_and_autograd(geo):
    """distinct values: the library's indices and gradient are unambiguous"""
    K, s, p = geo
    g = torch.Generator().manual_seed(K * 100 + s * 10 + p)
    for (H, W) in U.SIZES[geo]:
        N, C = 2, 8
        x = torch.randperm(N * H * W * C, generator=g).double().sub(N * H * W * C // 2).reshape(N, H, W, C)
        best, arg = U.pool_fwd64(x, K, s, p)
        xa = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        y, ind = F.max_pool2d(xa, K, s, p, return_indices=True)
        assert torch.equal(best, y.detach().permute(0, 2, 3, 1))
        h, w = U.arg_hw(arg, K, s, p)
        assert torch.equal(h * W + w, ind.permute(0, 2, 3, 1))
        dy = torch.randint(-100, 101, best.shape, generator=g).double()
        y.backward(dy.permute(0, 3, 1, 2))
        assert torch.equal(U.pool_bwd64(dy, arg, H, W, K, s, p), xa.grad.permute(0, 2, 3, 1))
        # the fused ReLU is the library's backward of the masked gradient
        yp = U.draw(U.relu_alphabet(F32), best.shape, g).double()
        xa.grad = None
        y2 = F.max_pool2d(xa, K, s, p)
        y2.backward(torch.where(yp > 0, dy, 0.0).permute(0, 3, 1, 2))
        assert torch.equal(U.pool_bwd64(dy, arg, H, W, K, s, p, yp), xa.grad.permute(0, 2, 3, 1))


def test_oracle_rules_for_ties_nan_and_empty_windows():
    """3 x 3 / 2 pad 1 on one 3 x 3 channel each: the documented rule, spelled out"""
    nan, inf = U.NAN, U.INF

    def arg00(rows):
        x = torch.tensor(rows, dtype=torch.float64).reshape(1, 3, 3, 1)
        return U.pool_fwd64(x, 3, 2, 1)[1].reshape(-1).tolist()

    # windows (0,0) (0,1) (1,0) (1,1): taps of rows / columns -1..1 and 1..3
    assert arg00([[1, 1, 0], [1, 1, 0], [0, 0, 0]]) == [4, 3, 1, 0]          # equal values keep the first
    assert arg00([[-0.0, 0.0, 0], [0.0, -0.0, 0], [0, 0, 0]])[0] == 4        # -0.0 against +0.0 too
    assert arg00([[5, nan, 0], [nan, 9, 0], [0, 0, 0]])[0] == 5              # a NaN wins, the first NaN stays
    assert arg00([[-inf] * 3] * 3) == [4, 3, 1, 0]                           # nothing above -inf: the first in-range tap
    assert arg00([[-inf, -inf, 0], [-inf, inf, 0], [0, 0, 0]])[0] == 8


PARTS = {"pool-bf16": lambda: U.pool_cases(dts=("bf16",)), "pool-f32": lambda: U.pool_cases(dts=("f32",)),
         "special": U.special_cases, "planes": U.planes_cases, "rb-bf16": lambda: U.rb_cases(dts=("bf16",)),
         "rb-f32": lambda: U.rb_cases(dts=("f32",))}


@pytest.mark.parametrize("part", PARTS)
def test_generators_meet_their_exactness_bounds(part):
    """Every generator asserts what its case relies on: windows with tied maxima, dx sums exact in
    fp32 that land on bf16 ties where windows overlap, stored dx columns below 2^24 units, planes that
    carry their value."""
    cases = PARTS[part]()
    for c in cases:
        d, o = U.gen_pool(c)
        if c["op"] == "planes":
            U.planes_ref(o["y"].double().reshape(-1), c["bound"])
    assert len({key(c) for c in cases}) == len(cases)
    if part == "pool-bf16":
        assert sum(U.expects_ties(c) for c in cases) >= 40


def test_cap_and_avg_generators():
    for c in U.cap_cases():
        d = U.gen_cap(c)
        assert int(d["idx"].max()) == c["K"] ** 2 - 1
    for c in U.avg_cases():
        assert U.gen_avg(c).shape == (c["N"], c["C"])
    assert len({key(c) for c in U.avg_cases()}) == 48


def test_case_counts_and_coverage():
    pc = U.pool_cases()
    assert {(c["K"], c["s"], c["p"]) for c in pc} == {(3, 2, 1), (2, 2, 0), (3, 3, 0), (3, 1, 1), (5, 3, 2), (2, 1, 1),
                                                      (1, 1, 0), (15, 4, 7)}
    for geo in U.GEOS:
        K, s, p = geo
        mine = [c for c in pc if (c["K"], c["s"], c["p"]) == geo]
        hw = {(c["H"], c["W"]) for c in mine}
        assert (K, K) in hw and ((9, 11) in hw) and (geo != (15, 4, 7) or (17, 17) in hw)
        assert s == 1 or any((H + 2 * p - K) % s and (W + 2 * p - K) % s for (H, W) in hw)
        assert {(c["dt"], c["C"]) for c in mine} == {(dt, C) for dt in U.DTS for C in (8, 24, 64, 520)}
        assert {c["N"] for c in mine} == {1, 3}
    # K == stride: every remainder of H, both backward kernels
    assert {c["H"] % 3 for c in pc if c["K"] == 3 and c["s"] == 3} == {0, 1, 2}
    assert {c["H"] % 2 for c in pc if c["K"] == 2 and c["s"] == 2} == {0, 1}
    assert U.bwd_variants(dict(K=2, s=2, p=0)) == (("part", 0), ("gather", 1))
    assert U.bwd_variants(dict(K=3, s=2, p=1)) == (("gather", 0),)
    # 15 x 15 on 17 x 17: argmax bytes up to 224
    c = next(c for c in pc if c["K"] == 15 and c["H"] == 17 and c["dt"] == "f32" and c["C"] == 8)
    assert int(U.gen_pool(c)[1]["idx"].max()) == 224
    rb = U.rb_cases()
    assert {c["C"] for c in rb} == {8, 16, 64, 512, 2048} and {c["db"] for c in rb} == {0, 1}
    assert {(c["K"], c["s"], c["p"], c["gather"]) for c in rb} >= {(3, 2, 1, 0), (2, 2, 0, 0), (2, 2, 0, 1)}
    cap = U.cap_cases()
    assert [U.partition(c) for c in cap] == [False, True]
    assert all(U.rb_threads(c) > 8192 * 256 for c in cap)
    sp = U.special_cases()
    assert {(c["K"], c["s"], c["p"], c["dt"]) for c in sp} == {(K, s, p, dt) for (K, s, p) in ((3, 2, 1), (2, 2, 0))
                                                               for dt in U.DTS}
    assert any(c["H"] == 1 and c["W"] == 1 for c in sp)  # the only in-range tap of its window
    assert {(c["N"], c["HW"], c["C"]) for c in U.avg_cases()} == {(N, HW, C) for N in (1, 3) for HW in (1, 4, 49, 64)
                                                                  for C in (8, 72, 256)}
    assert len(U.planes_cases()) == 8


def test_special_values_reach_the_windows():
    """the special-value input holds each special in a window's interior, at a border, twice in one
    window, and whole windows of -inf whose argmax is no padding tap"""
    c = dict(op="special", dt="f32", N=2, H=9, W=11, C=8, K=3, s=2, p=1)
    d, o = U.gen_pool(c)
    x, arg = d["x"], o["arg"]
    assert x[0, 0, 0, 0].isnan() and x[0, 4, 5, 0].isnan() and x[0, 4, 4, 0].isnan() and x[0, 8, 10, 0].isnan()
    assert (x[..., 5] == -U.INF).sum() == 2 * 99 - 1 and o["y"][..., 1].max() == U.INF
    assert int(arg[1, 0, 0, 5]) == 4 and int(arg[1, 0, 1, 5]) == 3 and int(arg[0, 0, 0, 7]) == 4
    assert o["y"][0, 2, 2, 5].isnan() and (o["y"][1, :, :, 5] == -U.INF).all()
    assert (o["y"][..., 4] == U.tiny(F32)).any() and (o["y"][..., 3] == 0).all()
    one = dict(c, H=1, W=1)
    assert U.gen_pool(one)[1]["arg"].unique().tolist() == [4]


def test_helpers_notice_one_byte_one_guard_one_tie_one_ulp():
    c = dict(op="pool", dt="bf16", N=1, H=9, W=11, C=8, K=3, s=2, p=1)
    d, o = U.gen_pool(c)
    Ho, Wo = U.out_hw(c)
    rows = Ho * Wo

    def result():
        res = {}
        for name, r, ref in (("y", rows, o["y"]), ("dx_gather", 99, o["dx"])):
            res[name], _ = out_buf(r, 8, BF16, "cpu")
            res[name][PRE:PRE + r] = ref.reshape(-1, 8).view(torch.int16)
        res["idx"], _ = byte_buf(rows * 8, "cpu")
        res["idx"][BPRE:BPRE + rows * 8] = o["idx"].reshape(-1)
        return res

    U.check_pool(c, result())
    # one flipped argmax byte
    bad = result()
    bad["idx"][BPRE + 17] ^= 1
    with pytest.raises(AssertionError, match="argmax"):
        U.check_pool(c, bad)
    # one touched guard byte / element
    for name, at in (("idx", BPRE - 1), ("idx", BPRE + rows * 8), ("dx_gather", (PRE + 99, 0)), ("y", (PRE - 1, 7))):
        bad = result()
        bad[name][at] = 0
        with pytest.raises(AssertionError):
            U.check_pool(c, bad)
    # one bf16 tie rounded the wrong way: the stored value one bf16 step off at a tie of the fp64 sum
    dx64 = U.pool_bwd64(d["dy"].double(), o["arg"], 9, 11, 3, 2, 1)
    ties = bf16_ties(dx64).reshape(-1).nonzero()
    assert ties.numel() > 0
    i = int(ties[0])
    mid, even = dx64.reshape(-1)[i], o["dx"].reshape(-1)[i].double()
    odd = (2 * mid - even).to(BF16)  # the other bf16 neighbour of the midpoint, as near as the right one
    assert odd.double() == 2 * mid - even and odd.double() != even
    bad = result()
    bad["dx_gather"].view(-1)[PRE * 8 + i] = odd.view(torch.int16)
    with pytest.raises(AssertionError, match="dx gather"):
        U.check_pool(c, bad)
    # one value 1 ulp off
    a = torch.tensor([1.0, 300.0])
    b = a.clone().view(torch.int32)
    b[1] += 1
    with pytest.raises(AssertionError):
        same_bits(a, b.view(F32), "u")
    # a store past the workspace
    g = torch.full((U.WPRE + U.WPOST,), U.SENT32, dtype=torch.int32)
    U.check_ws_guards(g, "w")
    g[U.WPRE] = 0
    with pytest.raises(AssertionError):
        U.check_ws_guards(g, "w")
    # the environment helper restores what it found
    import os
    with U.pool_env(1):
        assert os.environ.get("MPIT_POOL_GATHER") == "1"
    assert "MPIT_POOL_GATHER" not in os.environ


# ------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("dt", U.DTS)
@pytest.mark.parametrize("geo", U.GEOS, ids=lambda g: "k%ds%dp%d" % g)
def test_maxpool_exact(geo, dt):
    """maxpool_fwd then maxpool_bwd (the gather; K == stride: the per-window kernel and, under
    MPIT_POOL_GATHER, the gather) fed the oracle's bytes: y, argmax bytes and dx bitwise.
    9 x 11, one window, sizes that leave trailing pixels without a window; C = 8 .. 520, N = 1, 3."""
    _run(U.pool_cases(geos=(geo,), dts=(dt,)))


@gpu
def test_maxpool_backward_with_the_forwards_own_bytes():
    cases = [c for c in U.pool_cases(cs=(8, 64)) if (c["H"], c["W"]) in ((9, 11), (17, 17), (10, 9))]
    _run(cases, launch=lambda m, c: U.launch_pool(m, c, own=True))


@gpu
def test_maxpool_special_values():
    """NaN, +-inf, -0.0 / +0.0, subnormals and whole windows of -inf: interior, border, the only
    in-range tap, twice in one window (pool_exact_util._special_x)"""
    _run(U.special_cases())


@gpu
def test_maxpool_planes_output():
    """fp16 planes (obound): h and l halves from the documented formulas, the decoded value the
    chosen input itself, the 16 published bound slots"""
    _run(U.planes_cases())


@gpu
@pytest.mark.parametrize("dt", U.DTS)
def test_maxpool_bwd_fused_relu_bias(dt):
    """ypool / db: the overlapped 3 x 3 / 2 gather, the 2 x 2 / 2 and 3 x 3 / 3 per-window kernel and
    the gather on the same windows; C = 8 .. 2048 (one to 256 channel groups per block), with and
    without db; the workspace has exactly maxpool_bwd_ws_floats floats"""
    _run(U.rb_cases(dts=(dt,)))


@gpu
@pytest.mark.parametrize("kind", ("gather", "part"))
def test_maxpool_bwd_fused_past_the_block_cap(kind):
    """more threads than 8192 blocks hold: threads take a second pixel with the same 8 channels"""
    c = U.cap_cases()[kind == "part"]
    U.run_cap(_m(), c)


@gpu
def test_maxpool_bwd_rejects_what_it_cannot_run():
    m = _m()
    s = torch.cuda.current_stream().cuda_stream
    t = torch.zeros(1 << 16, device="cuda")
    p = t.data_ptr()

    def bwd(C, **kw):
        m.maxpool_bwd(0, s, 1, 4, 4, C, 2, 2, 0, p, p, p, f32=True, **kw)

    with pytest.raises(ValueError, match="workspace"):   # ypool without ws: nothing is launched
        bwd(8, ypool=p)
    with pytest.raises(ValueError, match="workspace"):
        bwd(8, ypool=p, db=p)
    with pytest.raises(ValueError, match="ypool"):
        bwd(8, db=p, ws=p)
    with pytest.raises(ValueError, match="256"):         # 256 % (24 / 8) != 0
        bwd(24, ypool=p, ws=p)
    with pytest.raises(ValueError, match="misaligned"):
        bwd(8, ypool=p + 4, ws=p)
    torch.cuda.synchronize()
    assert (t == 0).all()


@gpu
def test_avgpool_bwd_exact():
    """dy fp32(1 / HW): bitwise dy / HW for HW a power of two; HW = 49: the two-step emulation
    bitwise (bf16), within two roundings of fp64 (fp32)"""
    _run(U.avg_cases())
