"""The ResNet stem's BatchNorm + ReLU + max pool as one op each way on MI355X
(csrc/kernels/bn_act.hip ``bn_pool_fwd`` / ``bn_pool_bwd``).

``pool(relu(bn(x)))`` composed from :class:`BatchNormAct2d` and :class:`MaxPool2dNHWC` writes
the BN output and its ReLU mask only for the pool to read them, and the pool's input gradient
only for the two BN backward passes to read it — on the largest activation of the network.
Here the forward pools ``relu(x * scale + shift)`` straight from the convolution output, and
both BN backward passes gather the pool's gradient themselves and recompute the ReLU bit from
the x they read anyway. Each kernel repeats the arithmetic and the summation order of the
kernels it replaces, so every output (pooled values, argmax, statistics, dx, dgamma, dbeta and
the fp16x3 bounds) has the bits of the composition; ``_STEM_FUSE = False`` (``MPIT_STEM_FUSE=0``)
selects the composition for A/B runs and tests.

Measured on the ResNet-50 step (profiles/stem_fuse.md): fp32 0.9 % faster; bf16 autocast, whose
step is not bound by these kernels, showed no gain (between +0.15 % and -0.5 %). So the
default fuses fp32 steps only; ``MPIT_STEM_FUSE=1`` (``_STEM_FUSE = True``) fuses both.
"""
from __future__ import annotations

import os

import torch

from .._ext import native
from . import bn as _bn
from . import conv as _conv
from .bn import BatchNormAct2d, _amax_buf, _cl, _want_amax, tile_stats_of
from .conv import ReluLink, set_amax, set_planes
from .pool import MaxPool2dNHWC, _int

# MPIT_STEM_FUSE: "fp32" (default) fuses the stem of fp32 steps, 1 of fp32 and bf16 steps,
# 0 of none (bn1 and the max pool run as two modules). The attribute holds "fp32", True or False.
_STEM_FUSE = {"0": False, "1": True, "all": True}.get(os.environ.get("MPIT_STEM_FUSE", "fp32"), "fp32")

# how often the fused forward / backward ran (tests assert the fused path was taken)
COUNTERS = {"fwd": 0, "bwd": 0}


class _BNPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, k, stride, pad, tstats=None,
                amax=None, obound=None):
        x = _cl(x)
        n, c, h, w_ = x.shape
        M = n * h * w_
        m = native()
        dev = x.device.index
        stream = torch.cuda.current_stream(x.device).cuda_stream
        bf16 = x.dtype == torch.bfloat16
        f32 = dict(dtype=torch.float32, device=x.device)
        w = weight.float().contiguous() if weight is not None else None
        b = bias.float().contiguous() if bias is not None else None
        ts = tstats if (tstats is not None and tstats[1] == m.gemm_nt_tiles(M)) else None
        fold = ts[2] if ts is not None else None
        if ts is not None:
            _bn.COUNTERS["fwd_tile_stats"] += 1
        if fold is not None:  # the producing GEMM ran the finalize (and zeroed amax)
            _bn.COUNTERS["fwd_folded"] += 1
            mean, rstd, coef = fold.mean, fold.rstd, fold.coef
        else:  # coefficients only: statistics (or their tile finalize), running stats, amax zeroed
            mean, rstd = torch.empty(c, **f32), torch.empty(c, **f32)
            ws = torch.empty(m.bn_workspace_floats(c), **f32)
            m.bn_act_fwd(dev, stream, bf16, x.data_ptr(), 0, 0, M, c, w.data_ptr() if w is not None else 0,
                         b.data_ptr() if b is not None else 0,
                         running_mean.data_ptr() if running_mean is not None else 0,
                         running_var.data_ptr() if running_var is not None else 0, mean.data_ptr(), rstd.data_ptr(),
                         ws.data_ptr(), float(momentum), float(eps), False, 0,
                         stats=ts[0].data_ptr() if ts is not None else 0, nstat=ts[1] if ts is not None else 0,
                         amax=amax.data_ptr() if amax is not None else 0)
            coef = ws[: 2 * c]
        ho, wo = (h + 2 * pad - k) // stride + 1, (w_ + 2 * pad - k) // stride + 1
        y = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
        m.bn_pool_fwd(dev, stream, bf16, n, h, w_, c, k, stride, pad, x.data_ptr(), coef.data_ptr(), y.data_ptr(),
                      idx.data_ptr(), amax=amax.data_ptr() if amax is not None else 0)
        if obound is not None:
            # fp16 planes scaled by the exact max |relu(bn(x))| the pass above raised: a second,
            # small pass over the pooled values (a bound from the coefficients would be known
            # earlier but gives another exponent, so other low planes)
            yp = torch.empty_like(y, memory_format=torch.channels_last)
            m.pool_planes(dev, stream, y.data_ptr(), yp.data_ptr(), y.numel(), amax.data_ptr(), obound.data_ptr())
            y = yp
        ctx.save_for_backward(x, idx, coef, w, mean, rstd)
        ctx.geo = (k, stride, pad)
        ctx.has_w = weight is not None
        ctx.has_b = bias is not None
        COUNTERS["fwd"] += 1
        return y

    @staticmethod
    def backward(ctx, dy):
        x, idx, coef, w, mean, rstd = ctx.saved_tensors
        k, stride, pad = ctx.geo
        dy = _cl(dy).to(x.dtype)
        n, c, h, w_ = x.shape
        m = native()
        f32 = dict(dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        dgamma = torch.empty(c, **f32) if ctx.has_w else None
        dbeta = torch.empty(c, **f32) if ctx.has_b else None
        ws = torch.empty(m.bn_workspace_floats(c), **f32)
        amax = _amax_buf(x)  # max |dx|: the stem's weight gradient reads it
        m.bn_pool_bwd(x.device.index, torch.cuda.current_stream(x.device).cuda_stream, x.dtype == torch.bfloat16, n, h,
                      w_, c, k, stride, pad, dy.data_ptr(), idx.data_ptr(), x.data_ptr(), coef.data_ptr(),
                      w.data_ptr() if w is not None else 0, mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                      dgamma.data_ptr() if dgamma is not None else 0, dbeta.data_ptr() if dbeta is not None else 0,
                      ws.data_ptr(), amax=amax.data_ptr() if amax is not None else 0)
        if amax is not None:
            set_amax(dx, amax)
        COUNTERS["bwd"] += 1
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None


def fusable(bn, pool, x: torch.Tensor) -> bool:
    """True when ``pool(bn(x))`` runs as the fused op: a ReLU'd :class:`BatchNormAct2d` on its
    fused training path, a :class:`MaxPool2dNHWC` on its HIP path with no ReLU link on the
    input, and windows that cover every input pixel (then the maximum over the pooled values is
    the maximum over the BN output, the bound the composition publishes)."""
    if not (_STEM_FUSE and isinstance(bn, BatchNormAct2d) and isinstance(pool, MaxPool2dNHWC)):
        return False
    if _STEM_FUSE == "fp32" and x.dtype != torch.float32:
        return False
    if not (bn.act and bn.fused(x) and pool.fused(x) and ReluLink.of(x) is None):
        return False
    k, s, p = _int(pool.kernel_size), _int(pool.stride), _int(pool.padding)
    return bool(native().bn_pool_covered(x.shape[2], x.shape[3], k, s, p))


def bn_relu_pool(bn, pool, x: torch.Tensor) -> torch.Tensor:
    """``pool(bn(x))`` for a ReLU'd BN: one fused op each way when :func:`fusable`, the two
    modules otherwise. Same state updates, bounds and planes tag as the composition."""
    if not fusable(bn, pool, x):
        return pool(bn(x))
    momentum, rm, rv = bn._train_args()
    ts = tile_stats_of(x)
    fold = ts[2] if ts is not None else None
    # a folded finalize zeroed its own output bound (the pooling pass raises it)
    amax = fold.amax if (fold is not None and _want_amax(x)) else _amax_buf(x)
    planes = (pool.out_planes and _conv._F32_PLANES and x.dtype == torch.float32 and amax is not None
              and pool.training)
    ob = torch.empty(_conv.BOUND_FLOATS, dtype=torch.float32, device=x.device) if planes else None
    y = _BNPoolFn.apply(x, bn.weight, bn.bias, rm, rv, momentum, bn.eps, _int(pool.kernel_size), _int(pool.stride),
                        _int(pool.padding), ts, amax, ob)
    if ob is not None:
        set_planes(y, ob)
    elif amax is not None:  # every pooled value is one of the BN outputs: their bound holds
        set_amax(y, amax)
    return y
