"""Print, as JSON, the launch the GEMM planners choose for every case that
tests/gemm_plan_cases.py lists under whatever knobs the environment sets (they are read once per
process). No GPU is touched: dev = -1 plans for 256 compute units."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemm_plan_cases as G
from mpit_amd._ext import native

m = native()


def row(c):
    """One case as the table's row: instantiation | grid | LDS bytes (| split-reduce grids)."""
    M, N, K, C = c["M"], c["N"], c["K"], c["C"]
    try:
        if c["op"] == "nt":
            lda, ldb = (C or K), K
            p = m.gemm_nt_plan(f32=bool(c["f32"]), M=M, N=N, K=K, C=C, pitch=c["pitch"], ostr=c["ostr"], epi=c["epi"],
                               lda=lda, ldb=ldb, bps=N * ldb if c["bps"] else 0, amax_a=bool(c["amax"]),
                               amax_b=bool(c["amax"]), aps=M * lda + 64 if c["aps"] else 0)
            return "nt:%d:%d:%d:%d:%d:%d:%d|%d|%d" % tuple(
                p[k] for k in ("f32", "BM", "BN", "STAGES", "EPI", "CONV", "FM", "grid", "lds"))
        p = m.gemm_tn_plan(dev=-1, f32=bool(c["f32"]), M=M, N=N, K=K, C=C, pitch=c["pitch"], beta=float(c["beta"]),
                           ws=True, amax_y=bool(c["amax"]), amax_x=bool(c["amax"]),
                           yps=M * N + 64 if c["planes"] else 0, xps=M * K + 64 if c["planes"] else 0)
        if p["f32s"]:
            s = "tnf32s:%d:%d" % (p["f32"], p["CONV"])
        else:
            s = "tn:%d:%d:%d:%d:%d:%d:%d" % tuple(p[k] for k in ("f32", "TBN", "TBK", "STAGES", "CONV", "FM", "KR"))
        red = []
        if not p["direct"] and not p["fused"]:  # the split_reduce launches: (N K / 4 float4s / 256, groups)
            gx = (N * K // 4 + 255) // 256
            red = ["%d.%d" % (gx, p["groups"])] * bool(p["groups"]) + ["%d.1" % gx]
        return s + "|%d|%d|%s" % (p["grid"], p["lds"], ",".join(red))
    except ValueError as e:
        return "error:invalid_argument:" + str(e)
    except RuntimeError as e:
        return "error:logic_error:" + str(e)


json.dump({"rows": [row(c) for c in G.cases(os.environ)], "nt_built": m.gemm_nt_built(), "tn_built": m.gemm_tn_built()},
          sys.stdout)
