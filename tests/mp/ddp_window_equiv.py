"""Bucketed synchronous DP over the window all-reduce (parallel/ddp.py ``algo="window"``).

T_PART=grads (any rank count): random gradients (not exactly representable, so the order of
addition shows) through BucketedAllreduce with tiny buckets and with one bucket, fp32 and bf16
wire: bitwise equal to each other and to the left fold in rank order; padding untouched.
T_PART=train: four timed cnn7 steps (after one warm-up step) with optimizer="allreduce", tiny
buckets against one bucket, both on the window path: final parameters bitwise equal, and a
digest of them, which must agree across the ranks: every rank applies the same reduced bits.
T_PART=p2p (2 ranks: a sum of two is order-free): the same training on the window path and on
the point-to-point path: final parameters bitwise equal.
Prints one RESULT line from rank 0."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import mpit_amd as mp
from mpit_amd.models import get_model
from mpit_amd.parallel.ddp import BucketedAllreduce
from mpit_amd.train import TrainConfig, Trainer, timed_steps
from mpit_amd.utils.flat import FlatParams

# bitwise equality needs deterministic library kernels: cnn7's convolutions run on MIOpen,
# whose default backward-weight solvers may reduce with atomics
torch.backends.cudnn.deterministic = True
torch.backends.cudnn.benchmark = False
mp.Init()
W = mp.COMM_WORLD()
r, n = W.Get_rank(), W.Get_size()
parts = os.environ.get("T_PART", "grads").split(",")
dev = mp.runtime.device() or torch.device("cpu")
res = {}


def bits_equal(a, b):
    return bool(torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)))


def digest(t):
    return hashlib.sha1(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def train(mb, algo):
    tr = Trainer(TrainConfig(model="cnn7", batch=8, num_classes=10, optimizer="allreduce", lr=0.05, bucket_mb=mb,
                             ar_algo=algo))
    nb, registered = len(tr.ddp.buckets), len(tr.ddp._registered)
    s0 = W.ar_stats()
    timed_steps(tr, 4, 1)
    s1 = W.ar_stats()
    final = tr.flat.flat.detach().clone()
    tr.stop()
    return final, nb, registered, {k: s1[k] - s0[k] for k in s1}


if "grads" in parts:
    torch.manual_seed(5)
    model = get_model("cnn7", num_classes=10).to(dev)
    for wire in ("fp32", "bf16"):
        out = {}
        for name, mb in (("tiny", 0.02), ("one", 1e6)):
            fp = FlatParams(model)
            ar = BucketedAllreduce(model, fp, bucket_mb=mb, first_bucket_mb=0.01 if mb < 1 else 0.0, wire=wire,
                                   algo="window")
            s0 = W.ar_stats()
            vals = torch.randn(fp.numel, generator=torch.Generator().manual_seed(100 + r))
            fp.grad.zero_()
            for p, off in zip(fp.params, fp.offsets):
                fp.grad[off:off + p.numel()].copy_(vals[off:off + p.numel()])
            for b in range(len(ar.buckets)):  # as the backward hooks would, last bucket first
                ar._launch(len(ar.buckets) - 1 - b)
            ar.finish()
            s1 = W.ar_stats()
            out[name] = (fp.grad.detach().cpu().clone(), len(ar.buckets), len(ar._registered),
                         s1["window"] - s0["window"], s1["window_staged"] - s0["window_staged"])
            offs, nums, numel = list(fp.offsets), [p.numel() for p in fp.params], fp.numel
            ar.remove()
        mask = torch.zeros(numel, dtype=torch.bool)
        for off, k in zip(offs, nums):
            mask[off:off + k] = True
        gs = [torch.where(mask, torch.randn(numel, generator=torch.Generator().manual_seed(100 + q)),
                          torch.zeros(numel)) for q in range(n)]
        if wire == "bf16":  # cast per rank, fp32 accumulation in rank order, ONE rounding to bf16
            gs = [g.bfloat16().float() for g in gs]
        exp = gs[0]
        for g in gs[1:]:
            exp = exp + g
        if wire == "bf16":
            exp = exp.bfloat16().float()
        ta, tb = out["tiny"][0], out["one"][0]
        res["grads_" + wire] = {"same": bits_equal(ta, tb), "fold": bits_equal(ta, exp),
                                "padding": bool((ta[~mask] == 0).all()), "buckets": (out["tiny"][1], out["one"][1]),
                                "registered": out["tiny"][2], "window": out["tiny"][3] == out["tiny"][1],
                                "staged": out["tiny"][4]}
if "train" in parts:
    a, nba, rega, sa = train(0.02, "window")
    b, nbb, _, _ = train(1e6, "window")
    res["train"] = {"same": bits_equal(a, b), "buckets": (nba, nbb), "registered": rega, "calls": sa,
                    "digest": digest(a), "finite": bool(torch.isfinite(a).all())}
if "p2p" in parts:
    a, nba, _, sa = train(0.02, "window")
    b, _, _, sb = train(0.02, "p2p")
    res["p2p"] = {"same": bits_equal(a, b), "buckets": nba, "window_calls": sa, "p2p_calls": sb}
allr = W.allgather_obj(res)
if r == 0:
    print("RESULT", allr, flush=True)
mp.Finalize()
