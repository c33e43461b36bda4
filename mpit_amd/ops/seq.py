"""Forward-only fused sentence encoder and GESD scoring of the BiCNN tower
(csrc/kernels/seq.hip; the reference's tower and similarity, BiCNN/bicnn.lua:30-121).

The encodes that dominate a BiCNN job run without autograd: up to ``maxnegsample`` candidate
answers per training example in the negative-sampling scan, and everything the tester rank
does. For those, ``encode`` replaces Embedding -> Linear -> tanh -> Conv1d (MIOpen, with its
layout transposes) -> masked_fill -> max -> nan_to_num -> relu -> normalise with

* :func:`hidden_windows`: one kernel from the token ids to the im2col rows of the temporal
  convolution (embedding and linear outputs never reach HBM),
* the convolution as the fp32 ``ops.conv.gemm_nt`` against the packed weight
  (:func:`pack_conv_weight`, refilled on every call: the parameter server writes the flat
  parameters from native code without bumping ``_version``),
* :func:`max_norm`: masked max over time + bias + ReLU + L2 normalisation,

and :func:`gesd_gather` scores gathered row pairs in one pass per pair. Every reduction runs
in an order fixed by the row length, so a sentence's encoding and a pair's score are the same
bits in any batch. fp32, device tensors only, no autograd: the callers (models/bicnn.py) keep
PyTorch's path for everything else. ``COUNTERS`` tells which path ran.

:func:`per_example_grads` (csrc/kernels/seq_grad.hip) is the forward-plus-backward counterpart for
the parity rule (models/bicnn.py ``parity_grad_``, ``BiCNN(fused_grad=True)``): the same forward
kernels, bit for bit, with the arg-max kept, then the per-example gradients of the margin loss
written straight into the ``[n, flat.numel]`` matrix: no autograd, no dense embedding gradient."""
from __future__ import annotations

from typing import Optional

import torch

from .._ext import native

COUNTERS = {"encode_fused": 0, "encode_fallback": 0, "gesd_fused": 0, "gesd_fallback": 0,
            "pegrad_fused": 0, "pegrad_fallback": 0}


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _check(name: str, dev, **ts):
    for n, (t, dt) in ts.items():
        if t is None:
            continue
        if t.dtype != dt:
            raise TypeError(f"{name}: {n} must be {dt}, got {t.dtype}")
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{name}: {n} must live on {dev}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {n} must be contiguous")


def _ptr(t: Optional[torch.Tensor]) -> int:
    return t.data_ptr() if t is not None else 0


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def packed_shape(filters: int, hidden: int, k: int):
    """(Fp, Kp) of the packed convolution weight: the filters rounded up to 64, ``k * hidden``
    rounded up to 16 (what the fp32 ``gemm_nt`` tiles need)."""
    return round_up(filters, 64), round_up(k * hidden, 16)


def pack_conv_weight(weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv1d weight ``[F, H, k]`` -> ``Wp[Fp, Kp]`` with ``Wp[f][j*H + i] = weight[f][i][j]``;
    rows ``F..Fp-1`` and columns ``k*H..Kp-1`` are zero. With ``out`` (a zero-initialised
    ``[Fp, Kp]`` buffer whose pad stays untouched) one strided copy refills it. Pure torch."""
    F, H, k = weight.shape
    Fp, Kp = packed_shape(F, H, k)
    if out is None:
        out = torch.zeros((Fp, Kp), dtype=weight.dtype, device=weight.device)
    elif out.shape != (Fp, Kp) or out.dtype != weight.dtype or out.device != weight.device or not out.is_contiguous():
        raise ValueError("pack_conv_weight: out must be a contiguous [Fp, Kp] buffer like the weight")
    with torch.no_grad():
        out[:F, : k * H].unflatten(1, (k, H)).copy_(weight.detach().permute(0, 2, 1))
    return out


def hidden_windows(tok: torch.Tensor, E: torch.Tensor, Wh: torch.Tensor, bh: Optional[torch.Tensor], k: int,
                   Kp: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[B*T, Kp]`` fp32 im2col rows of the width-``k`` temporal convolution over
    ``tanh(linear(embedding(tok)))``: ``out[(b,t)][j*H + i]`` is hidden unit ``i`` of token
    ``(b, t+j)``; taps past the sentence end and columns ``k*H..Kp-1`` are exactly 0."""
    if tok.dim() != 2 or E.dim() != 2 or Wh.dim() != 2 or Wh.shape[1] != E.shape[1]:
        raise ValueError("hidden_windows: tok [B, T], E [V, D], Wh [H, D]")
    B, T = tok.shape
    D, H = E.shape[1], Wh.shape[0]
    if bh is not None and bh.shape != (H,):
        raise ValueError("hidden_windows: bh [H]")
    if Kp is None:
        Kp = round_up(k * H, 16)
    if k < 1 or Kp < k * H or B * T == 0:
        raise ValueError("hidden_windows: need k >= 1, Kp >= k * H and at least one token")
    if out is None:
        out = torch.empty((B * T, Kp), dtype=torch.float32, device=tok.device)
    elif out.shape != (B * T, Kp):
        raise ValueError("hidden_windows: out [B*T, Kp]")
    f32 = torch.float32
    _check("hidden_windows", tok.device, tok=(tok, torch.int64), E=(E, f32), Wh=(Wh, f32), bh=(bh, f32), out=(out, f32))
    native().seq_hidden_windows(tok.device.index, _stream(tok), tok.data_ptr(), B, T, E.data_ptr(), D, Wh.data_ptr(),
                                _ptr(bh), H, k, out.data_ptr(), Kp)
    return out


def max_norm(c: torch.Tensor, tok: torch.Tensor, k: int, pad_idx: int, bias: Optional[torch.Tensor], F: int,
             eps: float = 1e-10, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``c [B*T, ldc >= F]`` (row ``(b,t)`` = window ``t`` of sentence ``b``) -> ``[B, F]``:
    max over the valid windows (``t <= T-k`` and ``tok[b][t+k-1] != pad_idx``) + bias, ReLU
    (0 without a valid window), divided by ``max(L2 norm, eps)``."""
    if tok.dim() != 2 or c.dim() != 2 or c.shape[0] != tok.numel() or c.shape[1] < F or F < 1:
        raise ValueError("max_norm: tok [B, T], c [B*T, ldc >= F]")
    B, T = tok.shape
    if bias is not None and bias.shape != (F,):
        raise ValueError("max_norm: bias [F]")
    if out is None:
        out = torch.empty((B, F), dtype=torch.float32, device=c.device)
    elif out.shape != (B, F):
        raise ValueError("max_norm: out [B, F]")
    f32 = torch.float32
    _check("max_norm", c.device, c=(c, f32), tok=(tok, torch.int64), bias=(bias, f32), out=(out, f32))
    native().seq_max_norm(c.device.index, _stream(c), c.data_ptr(), c.shape[1], tok.data_ptr(), B, T, k, int(pad_idx),
                          _ptr(bias), F, float(eps), out.data_ptr())
    return out


def gesd_gather(q: torch.Tensor, cand: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
    """``out[r][c] = gesd(q[r], cand[idx[r][c]])`` for ``q [n, D]``, ``cand [m, D]``, int64
    ``idx [n, w]`` (trusted, like an indexing op's): ``[n, w]`` fp32."""
    if q.dim() != 2 or cand.dim() != 2 or idx.dim() != 2 or q.shape[1] != cand.shape[1] or idx.shape[0] != q.shape[0]:
        raise ValueError("gesd_gather: q [n, D], cand [m, D], idx [n, w]")
    n, w = idx.shape
    if out is None:
        out = torch.empty((n, w), dtype=torch.float32, device=q.device)
    elif out.shape != (n, w):
        raise ValueError("gesd_gather: out [n, w]")
    if n * w == 0:
        return out
    f32 = torch.float32
    _check("gesd_gather", q.device, q=(q, f32), cand=(cand, f32), idx=(idx, torch.int64), out=(out, f32))
    native().gesd_gather(q.device.index, _stream(q), q.data_ptr(), cand.data_ptr(), idx.data_ptr(), n, w, q.shape[1],
                         out.data_ptr())
    return out


def _packed_weight(model) -> torch.Tensor:
    """The model's persistent ``Wp`` buffer, refilled from the convolution weight as it is NOW
    (no ``_version`` caching: the parameter server writes the flat parameters natively)."""
    w = model.conv.weight
    F, H, k = w.shape
    buf = getattr(model, "_mpit_wp", None)
    if buf is None or buf.device != w.device or buf.shape != packed_shape(F, H, k) or buf.dtype != w.dtype:
        buf = None
    buf = pack_conv_weight(w, buf)
    model._mpit_wp = buf
    return buf


def encode(model, tok: torch.Tensor) -> torch.Tensor:
    """``model.encode(tok)`` of a :class:`mpit_amd.models.bicnn.BiCNN` on the fused kernels:
    tok ``[B, T]`` int64 on the GPU -> ``[B, filters]`` fp32 unit embeddings. No autograd."""
    from . import conv as C

    F, H, k = model.conv.weight.shape
    if model.conv.stride != (1,) or model.conv.padding != (0,) or model.conv.dilation != (1,) or model.conv.groups != 1:
        raise ValueError("seq.encode: a plain stride-1 Conv1d is expected")
    tok = tok.contiguous()
    wp = _packed_weight(model)
    win = hidden_windows(tok, model.embed.weight.detach(), model.hidden.weight.detach(),
                         model.hidden.bias.detach() if model.hidden.bias is not None else None, k, wp.shape[1])
    c = C.gemm_nt(win, wp)  # [B*T, Fp]
    out = max_norm(c, tok, k, model.pad_idx, model.conv.bias.detach() if model.conv.bias is not None else None, F,
                   model.norm.eps)
    COUNTERS["encode_fused"] += 1
    return out


def pack_conv_weight_t(weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv1d weight ``[F, H, k]`` -> ``WpT[Kp64, Fp]``, the transpose of :func:`pack_conv_weight`'s
    ``Wp`` with its rows rounded up to 64 (``gemm_nt``'s N): ``WpT[j*H + i][f] = weight[f][i][j]``,
    zero elsewhere. With ``out`` (a zero-initialised buffer whose pad stays untouched) one strided
    copy refills it. Pure torch."""
    F, H, k = weight.shape
    Fp, Kp = packed_shape(F, H, k)
    shape = (round_up(Kp, 64), Fp)
    if out is None:
        out = torch.zeros(shape, dtype=weight.dtype, device=weight.device)
    elif out.shape != shape or out.dtype != weight.dtype or out.device != weight.device or not out.is_contiguous():
        raise ValueError("pack_conv_weight_t: out must be a contiguous [round_up(Kp, 64), Fp] buffer like the weight")
    with torch.no_grad():
        out[: k * H, :F].unflatten(0, (k, H)).copy_(weight.detach().permute(2, 1, 0))
    return out


def _packed_weight_t(model) -> torch.Tensor:
    """The model's persistent ``WpT`` buffer, refilled on every call like ``Wp``."""
    w = model.conv.weight
    F, H, k = w.shape
    Fp, Kp = packed_shape(F, H, k)
    buf = getattr(model, "_mpit_wpt", None)
    if buf is None or buf.device != w.device or buf.shape != (round_up(Kp, 64), Fp) or buf.dtype != w.dtype:
        buf = None
    buf = pack_conv_weight_t(w, buf)
    model._mpit_wpt = buf
    return buf


def stack_sentences(q: torch.Tensor, a_pos: torch.Tensor, a_neg: torch.Tensor, pad_idx: int) -> torch.Tensor:
    """``[q; a_pos; a_neg]`` as one ``[3n, T]`` int64 batch, padded with ``pad_idx`` to the longest."""
    n = q.shape[0]
    if q.dim() != 2 or a_pos.dim() != 2 or a_neg.dim() != 2 or a_pos.shape[0] != n or a_neg.shape[0] != n:
        raise ValueError("per_example_grads: q [n, Tq], a_pos [n, Tp], a_neg [n, Tn]")
    T = max(q.shape[1], a_pos.shape[1], a_neg.shape[1])
    tok = torch.full((3 * n, T), int(pad_idx), dtype=torch.int64, device=q.device)
    for i, t in enumerate((q, a_pos, a_neg)):
        tok[i * n: (i + 1) * n, : t.shape[1]] = t
    return tok


def per_example_grads(model, flat, q: torch.Tensor, a_pos: torch.Tensor, a_neg: torch.Tensor, margin: float,
                      out: Optional[torch.Tensor] = None, parts: Optional[dict] = None):
    """``models.bicnn.per_example_grads`` on the fused kernels, forward and backward: returns
    ``(g, err)``, ``g`` ``[n, flat.numel]`` fp32 with row ``k`` the gradient of example ``k``'s margin
    loss alone (laid out like ``flat``: the parameters at ``flat.offsets``, zeros in the alignment gaps
    and in the embedding rows the example does not touch) and ``err`` ``[n]`` the per-example hinge
    values. No autograd inside (grad mode does not matter); the forward half is :func:`encode`'s and
    :func:`gesd_gather`'s bits. ``out``: a contiguous ``[n, flat.numel]`` buffer to use for ``g`` (it is
    zeroed first); ``parts``: a dict that receives the intermediates (tok, win, c, y, arg, den, sc, gy,
    dm, dc, dwin, da, de)."""
    from . import conv as C

    conv = model.conv
    F, H, k = conv.weight.shape
    if conv.stride != (1,) or conv.padding != (0,) or conv.dilation != (1,) or conv.groups != 1:
        raise ValueError("seq.per_example_grads: a plain stride-1 Conv1d is expected")
    E, Wh, bh, bc = model.embed.weight.detach(), model.hidden.weight.detach(), model.hidden.bias, conv.bias
    bh = bh.detach() if bh is not None else None
    bc = bc.detach() if bc is not None else None
    V, D = E.shape
    offs = {id(p): o for p, o in zip(flat.params, flat.offsets)}
    try:
        offE, offWh, offW = (offs[id(p)] for p in (model.embed.weight, model.hidden.weight, conv.weight))
        offBh = offs[id(model.hidden.bias)] if bh is not None else -1
        offB = offs[id(conv.bias)] if bc is not None else -1
    except KeyError:
        raise ValueError("seq.per_example_grads: flat does not hold the model's parameters") from None
    f32, dev = torch.float32, q.device
    with torch.no_grad():
        tok = stack_sentences(q, a_pos, a_neg, model.pad_idx)
        S, T = tok.shape
        n = S // 3
        if n == 0 or T == 0:
            raise ValueError("seq.per_example_grads: needs at least one example and one token")
        if out is None:
            g = torch.zeros((n, flat.numel), dtype=f32, device=dev)
        else:
            if out.shape != (n, flat.numel):
                raise ValueError("seq.per_example_grads: out [n, flat.numel]")
            g = out.zero_()
        _check("per_example_grads", dev, tok=(tok, torch.int64), E=(E, f32), Wh=(Wh, f32), bh=(bh, f32), bc=(bc, f32),
               out=(g, f32))
        m, st, di = native(), _stream(tok), dev.index
        # forward: encode()'s kernels, the arg-max and the clamped norm kept
        wp = _packed_weight(model)
        Fp, Kp = wp.shape
        win = hidden_windows(tok, E, Wh, bh, k, Kp)
        c = C.gemm_nt(win, wp)  # [S*T, Fp]
        y = torch.empty((S, F), dtype=f32, device=dev)
        arg = torch.empty((S, F), dtype=torch.int32, device=dev)
        den = torch.empty((S,), dtype=f32, device=dev)
        m.seq_max_norm_arg(di, st, c.data_ptr(), Fp, tok.data_ptr(), S, T, k, int(model.pad_idx), _ptr(bc), F,
                           float(model.norm.eps), y.data_ptr(), arg.data_ptr(), den.data_ptr())
        # scores, hinge and the gradient of the three encodings
        err = torch.empty((n,), dtype=f32, device=dev)
        sc = torch.empty((2, n), dtype=f32, device=dev)
        gy = torch.empty((S, F), dtype=f32, device=dev)
        m.gesd_pair_bwd(di, st, y.data_ptr(), n, F, float(margin), err.data_ptr(), sc.data_ptr(), gy.data_ptr())
        # through the normalisation, the ReLU and the max: one non-zero per (sentence, filter)
        dm = torch.empty((S, F), dtype=f32, device=dev)
        dc = torch.empty((S * T, Fp), dtype=f32, device=dev)
        m.seq_norm_max_bwd(di, st, gy.data_ptr(), y.data_ptr(), arg.data_ptr(), den.data_ptr(), S, T, F, Fp,
                           float(model.norm.eps), dm.data_ptr(), dc.data_ptr())
        dwin = C.gemm_nt(dc, _packed_weight_t(model))  # [S*T, round_up(Kp, 64)]
        m.seq_conv_wgrad_pe(di, st, dm.data_ptr(), arg.data_ptr(), win.data_ptr(), n, T, F, H, k, Kp, g.data_ptr(),
                            g.stride(0), offW, offB)
        da = torch.empty((S * T, H), dtype=f32, device=dev)
        de = torch.empty((S * T, D), dtype=f32, device=dev)
        m.seq_hidden_bwd(di, st, dwin.data_ptr(), dwin.shape[1], win.data_ptr(), Kp, S, T, H, k, Wh.data_ptr(), D,
                         da.data_ptr(), de.data_ptr())
        m.seq_hidden_embed_grad_pe(di, st, da.data_ptr(), de.data_ptr(), tok.data_ptr(), E.data_ptr(), V, n, T, H, D,
                                   int(model.pad_idx), g.data_ptr(), g.stride(0), offE, offWh, offBh)
    if parts is not None:
        parts.update(tok=tok, win=win, c=c, y=y, arg=arg, den=den, sc=sc, gy=gy, dm=dm, dc=dc, dwin=dwin, da=da, de=de)
    COUNTERS["pegrad_fused"] += 1
    return g, err
