"""The stem's fused BN + ReLU + max pool (csrc/kernels/bn_act.hip bn_pool_fwd / pool_planes /
bn_pool_bwd, ops/bn_pool.py) against the composition it replaces (bn_act_fwd -> maxpool_fwd;
maxpool_bwd -> bn_act_bwd): every comparison is bitwise."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

K, S, P = 3, 2, 1
MOM, EPS = 0.1, 1e-5


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _inputs(n, c, h, w, dt):
    """x, gamma, beta, g with the cases that separate a right kernel from a wrong one: a channel
    with negative gamma, a channel whose y is <= 0 everywhere (all masked), a block of equal
    values (ties take the first maximum) and, in bf16, values that tie only after rounding."""
    torch.manual_seed(n * 1000 + c * 10 + h)
    x = torch.randn(n, c, h, w, device="cuda")
    x[0, 3:5, 2:7, 2:7] = 2.0  # equal values: ties, and positive after the BN
    gamma = 0.5 + torch.rand(c, device="cuda")
    beta = 0.2 * torch.randn(c, device="cuda")
    gamma[1] = -1.25
    beta[2] = -50.0  # relu(bn(x)) == 0 on the whole channel
    gamma[5], beta[5] = 2.0 ** -10, 1.0  # y = 1 +- 0.003: distinct in fp32, equal as bf16
    x = _cl(x.to(dt))
    ho, wo = (h + 2 * P - K) // S + 1, (w + 2 * P - K) // S + 1
    g = _cl(torch.randn(n, c, ho, wo, device="cuda").to(dt))
    return x, gamma.contiguous(), beta.contiguous(), g


def _run(x, gamma, beta, g, fused):
    """Forward and backward through the native calls; fused: the new kernels, else the
    composition. Returns every quantity the two must agree on."""
    from mpit_amd._ext import native
    from mpit_amd.ops import conv as C

    m = native()
    n, c, h, w = x.shape
    M = n * h * w
    ho, wo = g.shape[2], g.shape[3]
    dev, st = x.device.index, torch.cuda.current_stream().cuda_stream
    bf16 = x.dtype == torch.bfloat16
    f32 = dict(dtype=torch.float32, device="cuda")
    rm, rv = torch.zeros(c, **f32), torch.ones(c, **f32)
    mean, rstd = torch.empty(c, **f32), torch.empty(c, **f32)
    ws = torch.empty(m.bn_workspace_floats(c), **f32)
    amax = None if bf16 else torch.empty(C.BOUND_FLOATS, **f32)
    ob = None if bf16 else torch.full((C.BOUND_FLOATS,), -1.0, **f32)
    ap = amax.data_ptr() if amax is not None else 0
    pooled = torch.empty((n, c, ho, wo), dtype=x.dtype, device="cuda", memory_format=torch.channels_last)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device="cuda")
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    dgamma, dbeta = torch.empty(c, **f32), torch.empty(c, **f32)
    ws2 = torch.empty(m.bn_workspace_floats(c), **f32)
    amax2 = None if bf16 else torch.empty(C.BOUND_FLOATS, **f32)
    ap2 = amax2.data_ptr() if amax2 is not None else 0
    if fused:
        m.bn_act_fwd(dev, st, bf16, x.data_ptr(), 0, 0, M, c, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                     rv.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), MOM, EPS, False, 0, amax=ap)
        m.bn_pool_fwd(dev, st, bf16, n, h, w, c, K, S, P, x.data_ptr(), ws.data_ptr(), pooled.data_ptr(),
                      idx.data_ptr(), amax=ap)
        if not bf16:
            plain = pooled
            pooled = torch.empty_like(plain, memory_format=torch.channels_last)
            m.pool_planes(dev, st, plain.data_ptr(), pooled.data_ptr(), plain.numel(), ap, ob.data_ptr())
        m.bn_pool_bwd(dev, st, bf16, n, h, w, c, K, S, P, g.data_ptr(), idx.data_ptr(), x.data_ptr(), ws.data_ptr(),
                      gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dgamma.data_ptr(),
                      dbeta.data_ptr(), ws2.data_ptr(), amax=ap2)
    else:
        y = torch.empty_like(x, memory_format=torch.channels_last)
        mask = torch.empty(m.bn_mask_bytes(bf16, M, c), dtype=torch.uint8, device="cuda")
        m.bn_act_fwd(dev, st, bf16, x.data_ptr(), 0, y.data_ptr(), M, c, gamma.data_ptr(), beta.data_ptr(),
                     rm.data_ptr(), rv.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), MOM, EPS, True,
                     mask.data_ptr(), amax=ap)
        m.maxpool_fwd(dev, st, n, h, w, c, K, S, P, y.data_ptr(), pooled.data_ptr(), idx.data_ptr(), f32=not bf16,
                      ibound=ap, obound=ob.data_ptr() if ob is not None else 0)
        dz = torch.empty_like(x, memory_format=torch.channels_last)
        m.maxpool_bwd(dev, st, n, h, w, c, K, S, P, g.data_ptr(), idx.data_ptr(), dz.data_ptr(), f32=not bf16)
        m.bn_act_bwd(dev, st, bf16, dz.data_ptr(), mask.data_ptr(), x.data_ptr(), dx.data_ptr(), 0, M, c,
                     gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                     ws2.data_ptr(), True, amax=ap2)
    torch.cuda.synchronize()
    out = dict(pooled=_bits(pooled.permute(0, 2, 3, 1)), idx=idx, mean=_bits(mean), rstd=_bits(rstd), rm=_bits(rm),
               rv=_bits(rv), dx=_bits(dx.permute(0, 2, 3, 1)), dgamma=_bits(dgamma), dbeta=_bits(dbeta))
    if not bf16:
        slots = lambda b: _bits(b.view(C.BOUND_SLOTS, C.BOUND_STRIDE)[:, 0])  # noqa: E731
        out.update(obound=slots(ob), ybound=_bits(C.bound_value(amax)), dxbound=_bits(C.bound_value(amax2)))
    return out


# (2,64,14,14): M = 392, two reduce blocks of 224 and 168 rows (paired loop and remainder);
# (1,64,9,11): odd, rectangular, clipped edge windows, one block; (3,16,12,12): G = 2, R = 128;
# (2,128,8,8): G = 16
SHAPES = [(2, 64, 14, 14), (1, 64, 9, 11), (3, 16, 12, 12), (2, 128, 8, 8)]


@gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_kernels_bitwise_equal_composition(shape, dt):
    """Pooled values (fp32: the planes' bytes and the published bound slots), argmax, saved and
    running statistics, dx, dgamma, dbeta and the dx bound: bit for bit the composition's."""
    x, gamma, beta, g = _inputs(*shape, dt)
    ref = _run(x, gamma, beta, g, fused=False)
    got = _run(x, gamma, beta, g, fused=True)
    assert ref.keys() == got.keys()
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    # the inputs do what they are meant to: a fully masked channel, ties taken by the first maximum
    assert int(got["dbeta"][2]) == 0 and int(got["dgamma"][2]) == 0  # sums of an all-zero dz: +0.0
    assert int(got["idx"][0, 2, 2, 3]) == 0 and int(got["idx"][0, 2, 2, 4]) == 0


@gpu
def test_fused_kernels_past_2_31_elements():
    """2 x 64 x 4100 x 4100 bf16 has 2^31 + 4 M elements: the kernels leave their 32-bit index
    arithmetic (multiply-shift divisions, 32-bit offsets) for the 64-bit one. Same comparison."""
    x, gamma, beta, g = _inputs(2, 64, 4100, 4100, torch.bfloat16)
    assert x.numel() > 2 ** 31
    ref = _run(x, gamma, beta, g, fused=False)
    got = _run(x, gamma, beta, g, fused=True)
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


@gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_uncovered_geometry_takes_the_composition(dt):
    """K=2, s=2, p=0 on an odd H leaves the last row in no window: the fused op is not taken (its
    bound argument needs every pixel in a window) and the result is the two modules'."""
    from mpit_amd._ext import native
    from mpit_amd.ops import bn_pool
    from mpit_amd.ops.bn import BatchNormAct2d
    from mpit_amd.ops.pool import MaxPool2dNHWC

    assert not native().bn_pool_covered(9, 9, 2, 2, 0)
    assert native().bn_pool_covered(9, 11, 3, 2, 1) and native().bn_pool_covered(112, 112, 3, 2, 1)
    torch.manual_seed(4)
    x0 = _cl(torch.randn(2, 16, 9, 9, device="cuda").to(dt))
    pool = MaxPool2dNHWC(2, stride=2)
    outs = []
    n0 = dict(bn_pool.COUNTERS)
    for composed in (False, True):
        torch.manual_seed(5)
        bn = BatchNormAct2d(16).cuda()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_()
        x = x0.clone().requires_grad_(True)
        y = pool(bn(x)) if composed else bn_pool.bn_relu_pool(bn, pool, x)
        y.backward(torch.ones_like(y))
        outs.append([y.detach(), x.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var])
    torch.cuda.synchronize()
    assert bn_pool.COUNTERS == n0
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(ValueError):  # refused by the geometry check, before any launch
        native().bn_pool_fwd(0, 0, dt == torch.bfloat16, 2, 9, 9, 16, 2, 2, 0, x0.data_ptr(), x0.data_ptr(),
                             x0.data_ptr(), x0.data_ptr())


@gpu
@pytest.mark.parametrize("fold", [False, True], ids=["finalize", "folded"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_resnet18_step_bitwise_with_and_without_the_fused_stem(dt, fold):
    """One training step of resnet18 (fp32 through the weight plan; bf16 autocast): the loss and
    every parameter gradient with the fused stem are bit for bit those of the composition, and the
    fused path did run. folded: the BN forward finalizes run inside the producing GEMMs
    (MPIT_BN_FOLD_FWD), so the fused forward takes its coefficients from the fold."""
    from mpit_amd.models.resnet import resnet18
    from mpit_amd.ops import bn as bnmod
    from mpit_amd.ops import bn_pool
    from mpit_amd.ops import conv as C

    torch.manual_seed(0)
    net = resnet18(num_classes=10).cuda().to(memory_format=torch.channels_last)
    x = _cl(torch.randn(4, 3, 64, 64, device="cuda"))
    tgt = torch.randint(0, 10, (4,), device="cuda")
    plan = C.WeightCastPlan(net, dt)

    def step():
        net.zero_grad(set_to_none=True)
        plan.run()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            out = net(x)
        loss = F.cross_entropy(out.float(), tgt)
        loss.backward()
        plan.invalidate()
        torch.cuda.synchronize()
        return [loss.detach().clone()] + [p.grad.clone() for p in net.parameters()]

    old = bn_pool._STEM_FUSE, bnmod._FWD_FOLD
    try:
        bnmod._FWD_FOLD = fold
        bn_pool._STEM_FUSE = False
        n0, f0 = dict(bn_pool.COUNTERS), bnmod.COUNTERS["fwd_folded"]
        ref = step()
        assert bn_pool.COUNTERS == n0
        assert (bnmod.COUNTERS["fwd_folded"] > f0) == fold
        bn_pool._STEM_FUSE = True
        got = step()
        assert bn_pool.COUNTERS["fwd"] == n0["fwd"] + 1 and bn_pool.COUNTERS["bwd"] == n0["bwd"] + 1
    finally:
        bn_pool._STEM_FUSE, bnmod._FWD_FOLD = old
    assert torch.isfinite(ref[0])
    for a, b in zip(ref, got):
        assert torch.equal(_bits(a), _bits(b))
