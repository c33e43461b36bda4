"""The exact-result BatchNorm cases of tests/bn_exact_util.py (worker_cases) under whatever knobs
the environment sets (MPIT_BN_APPLY_U, MPIT_BN_SPLIT, MPIT_BN_FIN_LANES: read once per process);
every buffer, guards included, saved to argv[1]. tests/test_bn_exact.py compares them with the
fp64 CPU oracles."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import bn_exact_util as U
from mpit_amd._ext import native

t0 = time.time()
m = native()
out = {}
for c in U.worker_cases(os.environ):
    for name, t in U.LAUNCH[c["op"]](m, c).items():
        out[U.key(c) + "|" + name] = t
torch.cuda.synchronize()
torch.save(out, sys.argv[1])
print("saved", len(out), f"{time.time() - t0:.1f}s")
