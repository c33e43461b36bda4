"""Shapes and knob settings of the GEMM selection table (tests/test_gemm_plan.py).

A case is the input of a planner query (`_mpit.gemm_nt_plan` / `_mpit.gemm_tn_plan`): the
element type, M, N, K, the geometry fields the choice depends on and which optional operands
are present. `cases()` is a fixed, ordered list; tests/golden/gemm_plan_table.json holds the
launch each case led to on the commit before the planners existed, per knob setting."""

BATCH = 256  # bench.py's per-GPU batch
EPI_NONE, EPI_STATS, EPI_BNRED, EPI_BNRED2, EPI_RELUB = range(5)


def nt(f32, M, N, K, C=0, pitch=0, ostr=1, epi=0, bps=0, amax=0, aps=0):
    return dict(op="nt", f32=f32, M=M, N=N, K=K, C=C, pitch=pitch, ostr=ostr, epi=epi, bps=bps, amax=amax, aps=aps)


def tn(f32, M, N, K, C=0, pitch=0, beta=0, amax=0, planes=0):
    return dict(op="tn", f32=f32, M=M, N=N, K=K, C=C, pitch=pitch, beta=beta, amax=amax, planes=planes)


# fp32 operand sets of gemm_nt: plain, bf16 B planes, fp16 B planes, fp16 A and B planes
F32_NT = (dict(), dict(bps=1), dict(bps=1, amax=1), dict(bps=1, amax=1, aps=1))
# gemm_tn: bf16, fp32 bf16x6, fp32 fp16x3, fp32 operands given as fp16 planes
TN_SETS = (dict(f32=0), dict(f32=1), dict(f32=1, amax=1), dict(f32=1, amax=1, planes=1))


def _nt_all(M, N, K, C, epis, pitch=0, ostr=1):
    """Every operand set of gemm_nt (the cross product is for the edge shapes)."""
    out = []
    for epi in epis:
        if K % 32 == 0:
            out.append(nt(0, M, N, K, C, pitch, ostr, epi))
        for s in F32_NT:
            if (pitch and s.get("aps")) or (K % 32 and s):
                continue  # (A planes are not for the row-tap stem; planes need K % 32 == 0)
            out.append(nt(1, M, N, K, C, pitch, ostr, epi, **s))
    return out


def _nt_step(M, N, K, C, epi, pitch=0, ostr=1):
    """A model's GEMM as the bf16 step and the fp32 step (A and B as fp16 planes) run it."""
    return [nt(0, M, N, K, C, pitch, ostr, epi), nt(1, M, N, K, C, pitch, ostr, epi, bps=1, amax=1, aps=1)]


def _tn_step(M, N, K, C=0, pitch=0):
    return [tn(M=M, N=N, K=K, C=C, pitch=pitch, **s) for s in (TN_SETS[:3] if pitch else (TN_SETS[0],) + TN_SETS[2:])]


def _conv_layer(B, hin, ci, co, k, stride):
    """Forward (BN statistics), backward-data (BN reduction) and backward-weight of one layer."""
    ho = hin // stride
    mo, mi = B * ho * ho, B * hin * hin
    if k == 1:  # (strided 1x1: a plain GEMM over the subsampled rows)
        return _nt_step(mo, co, ci, 0, EPI_STATS) + _nt_step(mo, ci, co, 0, EPI_BNRED) + _tn_step(mo, co, ci)
    out = _nt_step(mo, co, k * k * ci, ci, EPI_STATS)
    if stride == 1:
        out += _nt_step(mi, ci, k * k * co, co, EPI_BNRED)
    else:  # one parity class of the strided backward-data: ceil(k/2)^2 taps at most
        t = (k + 1) // 2
        out += _nt_step(mo, ci, t * t * co, co, EPI_BNRED, ostr=stride)
    return out + _tn_step(mo, co, k * k * ci, ci)


def _resnet50(B):
    out = []
    hin, cin = 56, 64
    for (mid, blocks, stride) in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for b in range(blocks):
            st = stride if b == 0 else 1
            out += _conv_layer(B, hin, cin, mid, 1, 1)
            out += _conv_layer(B, hin, mid, mid, 3, st)
            out += _conv_layer(B, hin // st, mid, mid * 4, 1, 1)
            if b == 0:
                out += _conv_layer(B, hin, cin, mid * 4, 1, st)
            hin, cin = hin // st, mid * 4
    # the paired BN reduction of a block's last 1x1 and its downsample, the residual ReLU fused
    out += _nt_step(B * 56 * 56, 64, 256, 0, EPI_BNRED2) + _nt_step(B * 56 * 56, 64, 9 * 64, 64, EPI_RELUB)
    # classifier: 1000 classes padded to 1024
    out += _nt_step(B, 1024, 2048, 0, EPI_NONE) + _nt_step(B, 2048, 1024, 0, EPI_NONE) + _tn_step(B, 1024, 2048)
    return out


def _stems(B):
    out = []
    # ResNet-50 stem: 8 kernel rows of 8 pixels x 4 channels, 112 x 112 outputs; VGG-16's first
    # layer: 3 rows (4 in the wgrad), 224 x 224 outputs
    for (ho, rows) in ((112, 8), (224, 3)):
        M = B * ho * ho
        out += _nt_all(M, 64, rows * 32, 32, (EPI_NONE, EPI_STATS), pitch=4)
        out += _tn_step(M, 64, (rows + (rows & 1)) * 32, 32, pitch=4)
    return out


def _vgg16(B):
    out = []
    for (h, ci, co) in ((112, 64, 128), (112, 128, 128), (56, 128, 256), (56, 256, 256)):
        M, K = B * h * h, 9 * ci
        out += _nt_step(M, co, K, ci, EPI_NONE) + _nt_step(M, ci, 9 * co, co, EPI_NONE) + _tn_step(M, co, K, ci)
    out += _nt_step(B, 4096, 25088, 0, EPI_NONE) + _nt_step(B, 25088, 4096, 0, EPI_NONE) + _tn_step(B, 4096, 25088)
    return out


def _bicnn():
    # sentence encoder: [S * T, k * emb] x [hidden, k * emb]^T and its backward
    out = []
    for (M, N, K) in ((128 * 40, 512, 3 * 128), (128 * 40, 3 * 128, 512), (64 * 200, 256, 2 * 96)):
        out += _nt_all(M, N, K, 0, (EPI_NONE,)) + [tn(M=M, N=N, K=K - K % 64, **s) for s in TN_SETS]
    return out


def _edges():
    out = []
    # every operand set and epilogue at each ring depth (K / k-tile = 1, 2, 3, 4) and column tile
    for N in (64, 128):
        for K in (16, 32, 48, 64, 96, 128):
            out += _nt_all(129, N, K, 0, (EPI_NONE, EPI_STATS, EPI_BNRED, EPI_BNRED2))
    for (M, N, K) in ((1, 64, 64), (1, 128, 128), (4096, 192, 64), (4096, 256, 128), (129, 256, 2304)):
        out += _nt_all(M, N, K, 0, (EPI_NONE, EPI_STATS, EPI_BNRED, EPI_BNRED2))
    # convolutions whose channels are no multiple of 64 / 128 (k-tile and ring-depth edges)
    for C in (32, 96, 128):
        for N in (64, 128):
            out += _nt_all(129, N, 9 * C, C, (EPI_NONE, EPI_STATS, EPI_BNRED, EPI_RELUB))
    out += _nt_all(129, 256, 9 * 256, 256, (EPI_NONE, EPI_STATS, EPI_BNRED, EPI_RELUB))
    # gemm_tn: one split, a few, more than one reduce group (two levels), with beta
    for M in (1, 129, 10000, 802816, 3211264):
        for (N, K) in ((64, 64), (64, 128), (128, 64), (128, 128), (192, 320)):
            out += [tn(M=M, N=N, K=K, beta=int(M in (129, 802816)), **s) for s in TN_SETS]
    for C in (64, 128, 192):
        out += [tn(M=M, N=N, K=9 * C, C=C, **s) for s in TN_SETS for (M, N) in ((129, 128), (100352, 64))]
    return out


def _no_planes(env):
    """Builds without the pre-split kernels: nt_plan refuses every case with B planes there."""
    return env.get("MPIT_F32_MFMA") == "native" or env.get("MPIT_F32_BK") == "16" or "MPIT_F32_ABLATE" in env


def cases(env=None):
    """The cases planned under the knobs `env`: all of them, except that where B planes are
    refused only those of one edge shape stay (the refusal itself is part of the table)."""
    seen, out = set(), []
    for c in _resnet50(BATCH) + _vgg16(BATCH) + _stems(BATCH) + _bicnn() + _edges():
        k = tuple(sorted(c.items()))
        if k not in seen:
            seen.add(k)
            out.append(c)
    if env and _no_planes(env):
        out = [c for c in out if not c.get("bps") or (c["M"], c["N"], c["K"], c["C"]) == (129, 128, 64, 0)]
    return out


# one setting per knob of GemmKnobs (csrc/kernels/gemm.hip), the default first
SETTINGS = (
    {},
    {"MPIT_GEMM_TILE": "128"}, {"MPIT_GEMM_TILE": "256x128"}, {"MPIT_GEMM_TILE": "256"},
    {"MPIT_GEMM_DEEPK": "0"}, {"MPIT_GEMM_DEEPK": "512"},
    {"MPIT_GEMM_STAGES": "3"}, {"MPIT_GEMM_STAGES": "4"},
    {"MPIT_F32_TILE": "256x128"}, {"MPIT_F32_TILE": "256x64"},
    {"MPIT_F32_MFMA": "native"}, {"MPIT_F32_BK": "16"},
    {"MPIT_F32_ABLATE": "nosplit"}, {"MPIT_F32_ABLATE": "splitA"}, {"MPIT_F32_ABLATE": "splitB"},
    {"MPIT_F32_WAVES": "2x2"}, {"MPIT_F32_NT": "acc1"},
    {"MPIT_F32_STAGES": "2"}, {"MPIT_F32_STAGES": "3"}, {"MPIT_F32_STAGES": "4"},
    {"MPIT_F32_BN64": "1"},
    {"MPIT_TN_OCC": "1"}, {"MPIT_TN_SPLIT_MUL": "2"}, {"MPIT_TN_SPLIT_DIV": "2"}, {"MPIT_TN_MIN_ROWS": "4096"},
    {"MPIT_TN_FUSED": "1"}, {"MPIT_TN_F16S": "0"}, {"MPIT_GEMM_TN_STAGES": "2"}, {"MPIT_TN_F32S": "1"},
    {"MPIT_TN_KROWS": "32"}, {"MPIT_TN_KROWS": "64"}, {"MPIT_TN_KR_STAGES": "3"},
    {"MPIT_GEMM_LOG": "1"},
    # knobs that only act next to another one
    {"MPIT_F32_BK": "16", "MPIT_F32_STAGES": "2"}, {"MPIT_F32_BK": "16", "MPIT_F32_STAGES": "3"},
    {"MPIT_F32_MFMA": "native", "MPIT_F32_BN64": "1"}, {"MPIT_F32_MFMA": "native", "MPIT_F32_TILE": "256x128"},
    {"MPIT_F32_MFMA": "native", "MPIT_F32_STAGES": "2"}, {"MPIT_F32_MFMA": "native", "MPIT_F32_STAGES": "3"},
    {"MPIT_F32_BK": "16", "MPIT_GEMM_STAGES": "4"}, {"MPIT_F32_BK": "16", "MPIT_F32_TILE": "256x128"},
    {"MPIT_TN_KROWS": "32", "MPIT_GEMM_TN_STAGES": "2"}, {"MPIT_TN_KROWS": "32", "MPIT_TN_OCC": "1"},
    {"MPIT_TN_KROWS": "32", "MPIT_TN_FUSED": "1"},
)


def base_of(env):
    """The setting a table entry is stored against: the first knob alone for a combination of
    two, else the default."""
    return dict([next(iter(env.items()))]) if len(env) > 1 else {}


def setting_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items()) or "default"
