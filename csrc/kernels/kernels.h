// Public C++ interface of the mpit HIP kernels (gfx950) and their host twins.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <array>
#include <map>
#include <string>
#include <vector>

namespace mpit {

// ---- fused elementwise update rules (updates.hip) --------------------------------
enum Rule : int {
  kApply = 0,        // K1   [p, g, (out)]                     sc: a
  kApplySum = 1,     // K1   [p, g0..g{NG-1}, (out)]           sc: a          variant |= NG << 8
  kRMSProp = 2,      // K2   [p, g, ga, gs, u, (out)]          sc: decay lr mom eps
  kAdam = 3,         // K3   [p, g, m, v, (out)]               sc: b1 b2 eps lr_t
  kAdamax = 4,       // K4   [p, g, m, u, (out)]               sc: b1 b2 eps lr_t
  kAdagrad = 5,      // K5   [p, g, var, (out)]                sc: eps clr
  kAdadelta = 6,     // K6   [p, g, var, acc, (out)]           sc: rho eps lr
  kNesterovPre = 7,  // K7   [vt, w]                           sc: mom
  kNesterovPost = 8, // K8   [w, g, vt, sug]                   sc: gscale l2wd clr
  kDownpour = 9,     // K9   [g, w, acc]                       sc: lr gscale l2wd  variant = mode
  kElastic = 10,     // K10  [w, c, sug]                       sc: mva
  kRegClip = 11,     // K11  [g, p]                            sc: gscale l1 l2 clip
  kScale = 12,       // K14  [x]                               sc: a
  kCopy = 13,        //      [dst, src]                        sc: a
  kFill = 14,        //      [dst]                             sc: v
  kAxpby = 15,       //      [y, x]                            sc: a b
};
enum Variant : int {
  kOut = 1 << 2,  // server rules: also write the new p to the last operand
  kAdd = 1 << 3,  // RMSProp: add u into p (global mode); otherwise produce u only (local)
  kVt = 1 << 4,   // Nesterov post: momentum buffer present
  kSug = 1 << 5,  // Nesterov post: fused EASGD "w -= sug"
};

// dev < 0 → host; else launch on `s` (device `dev`). bf = bitmask of bf16 operands.
void ew_update(int rule, int variant, int dev, hipStream_t s, int64_t n, const std::vector<uintptr_t>& ptrs,
               uint32_t bf, const std::vector<float>& sc);
// The same rule over several disjoint segments (ns[i] elements, operands ptrs[i]) in ONE
// launch (ew.h ew_multi_kernel); host, unaligned or > 16 segments: one pass per segment.
void ew_update_multi(int rule, int variant, int dev, hipStream_t s, const std::vector<int64_t>& ns,
                     const std::vector<std::vector<uintptr_t>>& ptrs, uint32_t bf, const std::vector<float>& sc);

// ---- reductions (reduce.hip) ------------------------------------------------------
// out[0] = Σ|x|, out[1] = Σx², out[2] = max|x|  (deterministic two-pass; `ws` holds
// kNormWsFloats floats of device scratch; ignored on host).
constexpr int kNormMaxBlocks = 1024;
constexpr int kNormWsFloats = 3 * kNormMaxBlocks;
void norms(int dev, hipStream_t s, const void* x, bool bf16, int64_t n, float* out, float* ws);
// out[0] = Σ x*y (fp32 accumulate), deterministic
void dot(int dev, hipStream_t s, const void* x, const void* y, bool bf16, int64_t n, float* out, float* ws);

// G[j] = clamp(G[j] + g[k][j] + l1*sign(p[j]) + l2*p[j], -c, c) for k = 0..n-1 in order
// (c <= 0: no clamp): the reference's per-example regularise + clamp of the accumulated
// gradient (BiCNN/bicnn.lua:398-409). g: n rows of stride ldg floats. fp32, dev < 0 = host.
void clamp_scan(int dev, hipStream_t s, float* G, const float* g, const float* p, int64_t P, int64_t ldg, int n,
                float l1, float l2, float c);

// ---- multi-tensor pack / unpack with cast (multi_copy.hip) ------------------------
struct CopyChunk {
  uint64_t src;    // byte address of the first element
  uint64_t dst;
  int64_t n;       // elements
  int32_t flags;   // bit0 src bf16, bit1 dst bf16
  int32_t pad;
};
// `table` = device (or host when dev < 0) array of `nchunks` CopyChunk. dst = scale*src.
void multi_copy(int dev, hipStream_t s, const CopyChunk* table, int64_t nchunks, float scale);

// ---- gradient gather + Downpour scale (gather.hip) ---------------------------------
// dst[off_t + i] = a*src_t[i] + b*aux[off_t + i]  (fp32; aux optional), one launch per
// kGatherMaxT tensors, table passed by value.
constexpr int kGatherMaxT = 128;
void gather_scale(int dev, hipStream_t s, const std::vector<uintptr_t>& srcs, const std::vector<int64_t>& offs,
                  const std::vector<int64_t>& ns, uintptr_t dst, uintptr_t aux, float a, float b);

// ---- fused BatchNorm (+residual) (+ReLU), NHWC, training (bn_act.hip) -------------
// x / res / y / dy / dx / dres: [M, C] row-major (channels_last), bf16 or fp32.
// mask: ReLU bit mask written by the forward (bn_mask_bytes: one byte per 8 channels, either
// dtype) and read by the backward. C % 8 == 0.
int64_t bn_workspace_floats(int C);
// fp16 planes output of an fp32 apply pass (the fp16x3 GEMMs then split nothing: gemm.hip
// FM 13). The pass writes h, l = the two fp16 planes of out * 2^e (h at element i, l at
// element i + numel of the 16-bit view of the output), e from a bound of |out| known BEFORE
// the pass: the maxima of its inputs (xmax / xmax2 / gmax: epoch slots a GEMM epilogue raised,
// gemm.hip EpiArgs::omax; rbound: the residual's bound) times its per-channel coefficients.
// obound (kBoundFloats) receives that bound in slot 0 (the other slots 0) for the consumers.
// rplanes: the residual arrives as planes (decoded with rbound's scale).
struct PlaneSpec {
  uintptr_t obound = 0;
  uintptr_t xmax = 0, xmax2 = 0, gmax = 0;
  uint32_t xep = 0, xep2 = 0, gep = 0;
  uintptr_t rbound = 0;
  int rplanes = 0;
};
int64_t bn_mask_bytes(bool bf16, int64_t M, int C);
// stats / nstat (optional): the statistics of x as per-128-row-tile (mean, M2) partials
// [nstat][2][C] emitted by the GEMM that produced x (EPI_STATS) — the statistics pass over
// x is skipped.
void bn_act_fwd(int dev, hipStream_t s, bool bf16, uintptr_t x, uintptr_t res, uintptr_t y, int64_t M, int C,
                uintptr_t gamma, uintptr_t beta, uintptr_t rmean, uintptr_t rvar, uintptr_t save_mean,
                uintptr_t save_rstd, uintptr_t ws, float momentum, float eps, bool relu, uintptr_t mask,
                uintptr_t stats = 0, int64_t nstat = 0, uintptr_t amax = 0, uintptr_t coef = 0,
                const PlaneSpec* planes = nullptr);
// amax (optional, fp32 [kBoundFloats], the slotted bound described at BnRed below): max |y| over
// the tensor (bn_act_bwd: max |dx|), taken from the fp32 values before a bf16 store rounds them,
// the scale bound of the fp16x3 GEMMs that read it: zeroed by this call's finalize (the tile
// finalize zeroes the kBoundSlots slot floats only, the stand-alone passes memset all
// kBoundFloats), raised by its apply pass with one atomic max per block, never lowered. With
// y / dx null (the coefficient-only calls of a bn_pair) amax is only zeroed, for the pair
// apply that follows. Given coefficients (bn_act_bwd coef), the GEMM that folded the finalize
// zeroed it (BnRed::fzero).
// y = act(x*coef[c] + coef[C+c] (+res))  — eval mode / precomputed coefficients
void bn_act_apply(int dev, hipStream_t s, bool bf16, uintptr_t x, uintptr_t res, uintptr_t y, int64_t M, int C,
                  uintptr_t coef, bool relu);
// part / npart (optional): (sum dz, sum dz*(x-mean)) partials [npart][2][C] already
// produced by the GEMM that wrote dy (EPI_BNRED) — the reduction pass is skipped.
void bn_act_bwd(int dev, hipStream_t s, bool bf16, uintptr_t dy, uintptr_t mask, uintptr_t x, uintptr_t dx,
                uintptr_t dres, int64_t M, int C, uintptr_t gamma, uintptr_t mean, uintptr_t rstd, uintptr_t dgamma,
                uintptr_t dbeta, uintptr_t ws, bool relu, uintptr_t part = 0, int64_t npart = 0,
                uintptr_t coef = 0, uintptr_t amax = 0, const PlaneSpec* planes = nullptr);
// coef (optional): the apply coefficients [3][C] already computed (the finalize folded into
// the GEMM that wrote dy, BnRed::fcoef; dgamma / dbeta written there too): apply pass only.

// bn_act_fwd with y == 0 / bn_act_bwd with dx == 0 only compute the coefficients into
// ws[0, 2C) (scale, shift) / ws[0, 3C) (A, C, B) and the running stats / dgamma, dbeta.
// A block's last BN and its downsample shortcut's BN as one op (bf16 or fp32, ReLU):
// y = relu(bn1(x1) + bn2(x2)) from the two forward coefficient sets, and the backward
// dx1 / dx2 from the two backward sets, one pass each.
void bn_pair_apply(int dev, hipStream_t s, uintptr_t x1, uintptr_t coef1, uintptr_t x2, uintptr_t coef2, uintptr_t y,
                   int64_t M, int C, uintptr_t mask, bool f32 = false, uintptr_t amax = 0, uintptr_t scratch = 0,
                   const PlaneSpec* planes = nullptr);
// amax / amax1 / amax2: raised by the pass (zeroed beforehand: the bn_act_fwd / bwd coefficient
// calls of the pair zero them); scratch: unused (kept for the call signature)
void bn_pair_bwd_apply(int dev, hipStream_t s, uintptr_t dy, uintptr_t mask, uintptr_t x1, uintptr_t coef1,
                       uintptr_t dx1, uintptr_t x2, uintptr_t coef2, uintptr_t dx2, int64_t M, int C, bool f32 = false,
                       uintptr_t amax1 = 0, uintptr_t amax2 = 0, uintptr_t scratch = 0,
                       const PlaneSpec* planes1 = nullptr, const PlaneSpec* planes2 = nullptr);

// ---- MFMA GEMMs for NHWC 1x1 convolutions (gemm.hip), fp32 accumulate -------------------
// Operands and outputs are bf16 (v_mfma_f32_32x32x16_bf16) or, with f32 = true, fp32
// (v_mfma_f32_32x32x2_f32: exact fp32 products). Everything said below of bf16 tensors holds
// for fp32 ones in an f32 call; ReLU bit masks are one byte per 8 channels either way.
// C[M,N] (bf16) = A[M,K] . B[N,K]^T; optional per-column (mean, M2) partials of C per
// 128-row tile into stats[ceil(M/128)][2][N] (gemm_nt_stats_floats); optional bf16 cin
// [M, ldc] (may alias C): the product is rounded to bf16 first, then cin is added and the sum
// rounded again — C = bf16(bf16(A.B^T) + cin), not bf16(A.B^T + cin) (fp32 calls: a single
// fp32 add); optional cmask (with cin, ldc == N): the bn_act ReLU bit mask of cin (1 byte /
// 8 channels) — adds cin*mask.
// Optional red: C is the output gradient of a bn_act layer (x, mask, mean its forward
// input / ReLU mask / batch mean, [.., N] like C): the GEMM also writes that layer's
// backward reduction partials (sum dz, sum dz*(x-mean)), dz = C*mask, one row pair per
// 128-row tile at part[row0 + tile][2][N] — bn_act_bwd(part, npart) then skips its pass.
// x2 / mean2 / part2 (optional): a second BN fed by the same gradient (the downsample
// shortcut's BN of a bn_pair): its (sum dz, sum dz*(x2-mean2)) go to part2.
// Output bounds (fp16x3 operand scales): kBoundSlots fp32 maxima kBoundStride floats apart
// (one 128-B line each, so the producers' one-atomic-per-block maxima spread over 16 lines
// instead of serialising on one address); the bound is the max over the slots.
constexpr int kBoundSlots = 16, kBoundStride = 32, kBoundFloats = kBoundSlots * kBoundStride;
struct BnRed {
  uintptr_t part = 0, x = 0, mask = 0, mean = 0;
  int64_t row0 = 0;
  uintptr_t part2 = 0, x2 = 0, mean2 = 0;
  // fold the BN backward's finalize into the GEMM (single EPI_BNRED launch): coefficients
  // [3][N], dgamma / dbeta [N], from gamma (or 0) and rstd; lvl: gemm_nt_fold_lvl_floats(N)
  uintptr_t fcoef = 0, fgamma = 0, frstd = 0, fdgamma = 0, fdbeta = 0, flvl = 0;
  // fp32 fp16x3 GEMMs (gemm.hip FM 11): device fp32 upper bounds of |A| and of |B|; amax_b
  // marks B (bps > 0) as the two fp16 planes of the weight scaled by its bound's 2^e
  uintptr_t amax_a = 0, amax_b = 0;
  // with fcoef: an output bound the folded finalize sets to zero (the BN backward's apply pass
  // then raises it to max |dx|)
  uintptr_t fzero = 0;
  // with the forward statistics (stats != 0): fold the BN forward's finalize into the GEMM
  // (single launch): scale / shift [2][N], save mean / rstd [N], running mean / var (or 0)
  // updated with momentum, from gamma / beta (or 0) and eps; lvl: gemm_nt_fold_lvl_floats(N);
  // zero: the BN output's bound, set to zero (the BN apply pass raises it)
  uintptr_t scoef = 0, sgamma = 0, sbeta = 0, srmean = 0, srvar = 0, smean = 0, srstd = 0, slvl = 0, szero = 0;
  float seps = 1e-5f, smom = 0.1f;
  // relu_y: instead of a BN reduction, the epilogue applies the ReLU of the conv(+bias)(+ReLU)
  // layer whose output x is this GEMM's input-gradient target: C = A.B^T * (x > 0) is that
  // layer's dz, and part[tile][0][N] its per-tile column sums (its bias gradient, col_sums)
  int relu_y = 0;
  // ftag: the fold's partials are (value, epoch) pairs (2 x the floats of part) in a buffer
  // that held only pairs of earlier launches (zeroed once, never garbage): the tagged fold
  // protocol of gemm.hip, in which no block waits for its own output stores
  int ftag = 0;
  // aps > 0 (with amax_b): A is two fp16 planes h, l of A * 2^e (e from amax_a), the l plane
  // aps elements after the h plane (gemm.hip FM 13: nothing split in the kernel)
  int64_t aps = 0;
  // omax (fp32 GEMMs): the launch's max |C| as 64-bit (epoch oepoch, value) maxima in kBoundSlots
  // slots kBoundStride floats apart (planes.h epoch_max reads them)
  uintptr_t omax = 0;
  uint32_t oepoch = 0;
};
int64_t gemm_nt_fold_lvl_floats(int N);
bool gemm_nt_supported(int64_t M, int N, int K, bool f32 = false);
int64_t gemm_nt_tiles(int64_t M);
int64_t gemm_nt_stats_floats(int64_t M, int N);
// bps > 0 (fp32 only): B is three pre-split bf16 planes h, m, l (x = h + m + l exactly, see
// cast_jobs kind flag 512) of bps elements each — the kernel splits only A in registers
void gemm_nt(int dev, hipStream_t s, int64_t M, int N, int K, uintptr_t A, int64_t lda, uintptr_t B, int64_t ldb,
             uintptr_t C, int64_t ldc, uintptr_t stats, uintptr_t cin, uintptr_t cmask = 0,
             const BnRed* red = nullptr, bool f32 = false, int64_t bps = 0);
// out[N,K] (fp32) = beta*out + Y[M,N]^T . X[M,K]  (split over M; ws: gemm_tn_ws_floats)
bool gemm_tn_supported(int64_t M, int N, int K);
int64_t gemm_tn_ws_floats(int dev, int64_t M, int N, int K);
// Read-only queries of the planners the launchers themselves call (gemm.hip nt_plan / tn_plan):
// the kernel instantiation, grid and dynamic LDS a call with these operands would run, as named
// fields; C / pitch / ostr are the ConvGeo's (C == 0: a plain GEMM), the strides and flags say
// which optional operands are present. Throws what the launch would throw for the combination.
// dev < 0: no GPU is touched (256 CUs). gemm_*_built: every instantiation that is compiled, as
// (f32, template arguments...).
std::map<std::string, int64_t> gemm_nt_plan(bool f32, int64_t M, int N, int K, int C, int pitch, int ostr, int epi,
                                            int64_t lda, int64_t ldb, int64_t bps, bool amax_a, bool amax_b,
                                            int64_t aps);
std::map<std::string, int64_t> gemm_tn_plan(int dev, bool f32, int64_t M, int N, int K, int C, int pitch, float beta,
                                            bool ws, bool amax_y, bool amax_x, int64_t yps, int64_t xps);
std::vector<std::vector<int>> gemm_nt_built();
std::vector<std::vector<int>> gemm_tn_built();
// compute units of device `dev`; a stream restricted to the CUs of `mask` (gemm.hip)
int device_cu_count(int dev);
uintptr_t stream_create_cu_masked(int dev, const std::vector<uint32_t>& mask);
// amax_y / amax_x (fp32, both or neither): device bounds of |Y|, |X| -> fp16x3 split products
void gemm_tn(int dev, hipStream_t s, int64_t M, int N, int K, uintptr_t Y, int64_t ldy, uintptr_t X, int64_t ldx,
             uintptr_t out, uintptr_t ws, float beta, bool f32 = false, uintptr_t amax_y = 0, uintptr_t amax_x = 0, int64_t yps = 0,
             int64_t xps = 0);
// fp32 w[R][T][Cc] -> bf16 wb[R][T][Cc] (optional) and bf16 tap-flipped transpose
// wt[Cc][T-1-t][R] (optional); T = 1 is the plain transpose
void cast_transpose(int dev, hipStream_t s, uintptr_t w, int R, int Cc, uintptr_t wb, uintptr_t wt, int taps = 1,
                    bool f32 = false);
// Many casts in one launch. Job spec: {kind, w, wb, wt, Co, C, R, S, stride, pad}, kind 0 =
// cast + tap-flipped transpose (conv_weights / cast_transpose), 1 = cast + strided
// parity-class weights (conv_dgrad_strided_weights), 2 = cast only. The table is built on the
// host (cast_job_bytes() per job) and uploaded once; cast_jobs_run launches it.
int64_t cast_job_bytes();
int64_t cast_jobs_build(uintptr_t host_table, const std::vector<std::array<int64_t, 11>>& specs);
void cast_jobs_run(int dev, hipStream_t s, uintptr_t dev_table, int njobs, int64_t nblocks, uintptr_t amax = 0);

// ---- NHWC RxS convolutions as implicit GEMMs on the same MFMA kernels ----------------
// x [Nb,H,W,C], w [Co,R,S,C] (bf16), y [Nb,Ho,Wo,Co] (bf16); stats / cin as gemm_nt.
// Backward-data of a stride-1 conv = conv_fwd(dy, wt, pad' = R-1-pad) with wt the
// tap-flipped transpose [C,R,S,Co] (cast_transpose taps = R*S).
bool conv_supported(int C, int Co);
// bias (fp32 [Co], optional) and ReLU are applied in the epilogue.
void conv_fwd(int dev, hipStream_t s, int Nb, int H, int W, int C, int Co, int R, int S, int stride, int pad,
              uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t stats, uintptr_t cin, uintptr_t bias = 0,
              bool relu = false, const BnRed* red = nullptr, bool f32 = false, int64_t bps = 0);
// ReLU + bias backward: dz = dy * (y > 0) (bf16 [M, C]), db[c] = sum_m dz (fp32, optional,
// deterministic); ws: relu_bias_bwd_ws_floats(C)
// Backward-data of a strided conv (stride 2..4) as stride^2 parity-class implicit GEMMs
// over dy; wcls = packed class weights (conv_dgrad_strided_wfloats bf16 elements) made by
// conv_dgrad_strided_weights from the fp32 master (also writes wb like cast_transpose).
int64_t conv_dgrad_strided_wfloats(int C, int Co, int R, int S, int stride, int pad);
void conv_dgrad_strided_weights(int dev, hipStream_t s, uintptr_t w, int Co, int C, int R, int S, int stride, int pad,
                                uintptr_t wb, uintptr_t wcls, bool f32 = false);
// partial rows a BN reduction over the strided backward-data writes (all classes)
int64_t conv_dgrad_strided_tiles(int Nb, int H, int W, int C, int Co, int R, int S, int stride, int pad);
void conv_dgrad_strided(int dev, hipStream_t s, int Nb, int H, int W, int C, int Co, int R, int S, int stride, int pad,
                        uintptr_t dy, uintptr_t wcls, uintptr_t dx, const BnRed* red = nullptr, bool f32 = false,
                        int64_t bps = 0);
// softmax cross-entropy over rows of logits x [rows][ldx] (bf16 or fp32; loss.hip): per-row
// loss (fp32 [rows]) and the logits' gradient d = (softmax - onehot) * scale (fp32 [rows][C])
void softmax_xent(int dev, hipStream_t s, int64_t rows, int C, uintptr_t x, int64_t ldx, bool bf16, uintptr_t tgt,
                  float scale, uintptr_t loss, uintptr_t d);

// ---- BiCNN sentence encoder and GESD scoring, forward only, fp32, device only (seq.hip) ----
// tok int64 [B][T] (ids trusted), E [V][D], Wh [H][D], bh [H] or 0 -> out fp32 [B*T][Kp], the im2col
// rows of a width-k temporal convolution: out[(b,t)][j*H + i] = tanh(bh[i] + E[tok[b][t+j]] . Wh[i])
// for t + j < T; missing taps and columns k*H .. Kp-1 are 0. Tap j of row (b,t) is bitwise tap 0
// of row (b,t+j).
void seq_hidden_windows(int dev, hipStream_t s, uintptr_t tok, int64_t B, int T, uintptr_t E, int D, uintptr_t Wh,
                        uintptr_t bh, int H, int k, uintptr_t out, int Kp);
// c fp32 [B*T][ldc >= F] (the convolution GEMM's output) -> out fp32 [B][F]: m = max(0, bias[f] +
// max over the valid windows t (t <= T-k and tok[b][t+k-1] != pad_idx) of c[(b,t)][f]), 0 without
// a valid window; out = m / max(|m|_2, eps). bias [F] or 0. The same bits for a sentence in any batch.
void seq_max_norm(int dev, hipStream_t s, uintptr_t c, int64_t ldc, uintptr_t tok, int64_t B, int T, int k,
                  int64_t pad_idx, uintptr_t bias, int F, float eps, uintptr_t out);
// q [n][D], cand [m][D], idx int64 [n][w] (trusted) -> out fp32 [n][w], the GESD similarity of q[r]
// and cand[idx[r][c]]: 1 / (1 + |a - b|_2) * 1 / (1 + exp(-(a . b + 1))). Independent of n and w.
void gesd_gather(int dev, hipStream_t s, uintptr_t q, uintptr_t cand, uintptr_t idx, int64_t n, int w, int D,
                 uintptr_t out);

// ---- BiCNN per-example gradients of the margin loss, fp32, device only (seq_grad.hip) ----
// S = 3n sentences [q; a_pos; a_neg] of a common T; sentence s belongs to example s % n. g is the
// [n][ldg] per-example gradient matrix, off* the parameters' offsets in a row (biases: -1 = none).
// Every reduction order is fixed by F, H, D, k and the example's own tokens.
// seq_max_norm + arg int32 [B][F] (the first valid window attaining the max; -1 without a valid
// window or with a ReLU output of 0) and den fp32 [B] (the clamped norm). out: seq_max_norm's bits.
void seq_max_norm_arg(int dev, hipStream_t s, uintptr_t c, int64_t ldc, uintptr_t tok, int64_t B, int T, int k,
                      int64_t pad_idx, uintptr_t bias, int F, float eps, uintptr_t out, uintptr_t arg, uintptr_t den);
// y [3n][F] -> sc [2][n] (sp = gesd(y[k], y[n+k]), sn = gesd(y[k], y[2n+k]): gesd_gather's bits),
// err [n] = max(0, (margin - sp) + sn), gy [3n][F] = d err / d y (zeros where err == 0).
void gesd_pair_bwd(int dev, hipStream_t s, uintptr_t y, int64_t n, int F, float margin, uintptr_t err, uintptr_t sc,
                   uintptr_t gy);
// dm [S][F] = arg >= 0 ? (gy - y * sum_f(gy * y)) / den : 0, and ALL of dc [S*T][Fp] (16-byte
// aligned, Fp % 4 == 0): dm[s][f] at row (s, arg[s][f]), zero elsewhere (pad columns included).
void seq_norm_max_bwd(int dev, hipStream_t s, uintptr_t gy, uintptr_t y, uintptr_t arg, uintptr_t den, int64_t S, int T,
                      int F, int Fp, float eps, uintptr_t dm, uintptr_t dc);
// g[k][offW + (f*H + i)*k + j] = sum over s = k, n+k, 2n+k (arg >= 0 only) of dm[s][f] *
// win[(s, arg[s][f])][j*H + i]; g[k][offB + f] = the sum of the three dm. win [S*T][Kp].
void seq_conv_wgrad_pe(int dev, hipStream_t s, uintptr_t dm, uintptr_t arg, uintptr_t win, int64_t n, int T, int F,
                       int H, int k, int Kp, uintptr_t g, int64_t ldg, int64_t offW, int64_t offB);
// da [S*T][H] = (1 - win[(s,t)][i]^2) * sum_{j<k, j<=t} dwin[(s,t-j)][j*H + i] (dwin [S*T][ldw]) and
// de [S*T][D] = Wh^T da per token.
void seq_hidden_bwd(int dev, hipStream_t s, uintptr_t dwin, int64_t ldw, uintptr_t win, int Kp, int64_t S, int T, int H,
                    int k, uintptr_t Wh, int D, uintptr_t da, uintptr_t de);
// Over example k's tokens in the order q, a_pos, a_neg, ascending t: g[k][offWh + i*D + d] = sum da[i] *
// E[tok][d], g[k][offBh + i] = sum da[i], g[k][offE + v*D + d] = sum of de over the occurrences of
// word v != pad_idx (each touched row written once; other rows of g are left alone). E [V][D].
void seq_hidden_embed_grad_pe(int dev, hipStream_t s, uintptr_t da, uintptr_t de, uintptr_t tok, uintptr_t E,
                              int64_t V, int64_t n, int T, int H, int D, int64_t pad_idx, uintptr_t g, int64_t ldg,
                              int64_t offE, int64_t offWh, int64_t offBh);
int64_t relu_bias_bwd_ws_floats(int C);
// out[c] = sum over rows k < nb of part[k * ld + c] (fp32, fixed order: deterministic); mid:
// col_sums_ws_floats(C) floats of workspace (needed when nb > 64)
int64_t col_sums_ws_floats(int C);
void col_sums(hipStream_t s, const float* part, int64_t nb, int64_t ld, int C, float* out, float* mid);
void col_sums(int dev, hipStream_t s, uintptr_t part, int64_t nb, int64_t ld, int C, uintptr_t out, uintptr_t mid);
void relu_bias_bwd(int dev, hipStream_t s, int64_t M, int C, uintptr_t dy, uintptr_t y, uintptr_t dz, uintptr_t db,
                   uintptr_t ws, bool f32 = false);
// dw [Co,R,S,C] (fp32) = beta*dw + dY^T . im2col(x)   (C % 64 == 0, Co % 64 == 0)
int64_t conv_wgrad_ws_floats(int dev, int Nb, int H, int W, int C, int Co, int R, int S, int stride, int pad);
void conv_wgrad(int dev, hipStream_t s, int Nb, int H, int W, int C, int Co, int R, int S, int stride, int pad,
                uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws, float beta, bool f32 = false,
                uintptr_t amax_y = 0, uintptr_t amax_x = 0, int64_t yps = 0,
                int64_t xps = 0);

// Row-tap stem conv (7x7 / stride-2 / 3-channel ResNet stem on MFMA; VGG's 3x3 / 3-channel
// first layer with rows = 3): x = zero-padded NHWC4 image [Nb][Hp][Wp][4], w = [Co][rows][8][4]
// (bf16, zero-extended kernel), y = [Nb][Ho][Wo][Co]; dw = [Co][rows_w][8][4] fp32 with rows_w =
// rows rounded up to even (the weight-gradient GEMM's K = rows_w * 32 must be a multiple of 64;
// the image then needs Hp >= (Ho - 1) * stride + rows_w); stats: BN statistics of y as conv_fwd;
// bias / relu: the conv(+bias)(+ReLU) epilogue of conv_fwd
void conv_stem_fwd(int dev, hipStream_t s, int Nb, int Hp, int Wp, int Co, int Ho, int Wo, int stride, uintptr_t x,
                   uintptr_t w, uintptr_t y, uintptr_t stats, bool f32 = false, int64_t bps = 0, uintptr_t amax_a = 0,
                   uintptr_t amax_b = 0, const BnRed* fold = nullptr, int rows = 8, uintptr_t bias = 0,
                   bool relu = false);
// (fp32 fp16x3: w as two fp16 planes of plane stride bps with bound amax_b, the image's bound amax_a;
// the wgrad's amax_y / amax_x as gemm_tn)
int64_t conv_stem_wgrad_ws_floats(int dev, int Nb, int Ho, int Wo, int Co, int rows = 8);
void conv_stem_wgrad(int dev, hipStream_t s, int Nb, int Hp, int Wp, int Co, int Ho, int Wo, int stride, uintptr_t dy,
                     uintptr_t x, uintptr_t dw, uintptr_t ws, bool f32 = false, uintptr_t amax_y = 0,
                     uintptr_t amax_x = 0, int rows = 8);
int stem_wgrad_rows(int rows);

// ---- NHWC bf16 / fp32 max pooling with a uint8 argmax per output element (pool.hip) ---
// x [N,H,W,C] -> y, idx [N,Ho,Wo,C]; dx [N,H,W,C] gathered from dy + idx (no atomics).
// obound (fp32, with ibound: x's slotted bound): y as fp16 planes (planes.h) scaled by x's bound
void maxpool_fwd(int dev, hipStream_t s, int N, int H, int W, int C, int K, int stride, int pad, uintptr_t x,
                 uintptr_t y, uintptr_t idx, bool f32 = false, uintptr_t ibound = 0, uintptr_t obound = 0);
// ypool (optional): the pool's output, when its input is a ReLU'd conv(+bias) output: dx is
// then that conv's dz = dx * (y > 0), and db (optional, fp32 [C]) its bias gradient; ws:
// maxpool_bwd_ws_floats(C) floats. Needs 256 % (C / 8) == 0.
void maxpool_bwd(int dev, hipStream_t s, int N, int H, int W, int C, int K, int stride, int pad, uintptr_t dy,
                 uintptr_t idx, uintptr_t dx, bool f32 = false, uintptr_t ypool = 0, uintptr_t db = 0,
                 uintptr_t ws = 0);
int64_t maxpool_bwd_ws_floats(int C);

// ---- stem: BN + ReLU + max pool as one op each way (bn_act.hip) ------------------------
// pool(relu(bn(x))) without the BN output, its ReLU mask or the pool's input gradient in memory.
// Only for windows that cover every input pixel (bn_pool_covered): then the maximum over the
// pooled values is the maximum over the BN output, today's bound.
bool bn_pool_covered(int H, int W, int K, int stride, int pad);
// x [N,H,W,C] (the conv output), coef [2][C] (scale, shift: bn_act_fwd with y == 0, or a
// folded finalize) -> y [N,Ho,Wo,C] plain bf16 / fp32 and idx as maxpool_fwd; amax (optional,
// zeroed by the finalize): raised to the exact max |relu(bn(x))|.
void bn_pool_fwd(int dev, hipStream_t s, bool bf16, int N, int H, int W, int C, int K, int stride, int pad,
                 uintptr_t x, uintptr_t coef, uintptr_t y, uintptr_t idx, uintptr_t amax = 0);
// fp32 x [nel] -> y as fp16 planes (planes.h) scaled by the slotted bound ibound, which obound
// receives in slot 0 (maxpool_fwd's planes output, from values already pooled)
void pool_planes(int dev, hipStream_t s, uintptr_t x, uintptr_t y, int64_t nel, uintptr_t ibound, uintptr_t obound);
// g [N,Ho,Wo,C]: the gradient of the pooled output; x, fcoef: the forward's; dx [N,H,W,C],
// dgamma, dbeta and amax (max |dx|) as bn_act_bwd with relu; ws: bn_workspace_floats(C).
// dz = the pool's gather (maxpool_bwd) masked by bn(x) > 0, computed in both passes instead of
// stored; the reduce pass adds in bn_act_bwd's order, so every output has its bits.
void bn_pool_bwd(int dev, hipStream_t s, bool bf16, int N, int H, int W, int C, int K, int stride, int pad,
                 uintptr_t g, uintptr_t idx, uintptr_t x, uintptr_t fcoef, uintptr_t gamma, uintptr_t mean,
                 uintptr_t rstd, uintptr_t dx, uintptr_t dgamma, uintptr_t dbeta, uintptr_t ws, uintptr_t amax = 0);
// global average pool backward over NHWC: dx[n][p][c] = dy[n][c] / HW (bf16 / fp32)
void avgpool_bwd(int dev, hipStream_t s, int N, int HW, int C, uintptr_t dy, uintptr_t dx, bool f32 = false);

// ---- peer reduce: the reducer of the window all-reduce (allreduce.hip) ---------------
// kPrOps counts the ten element-wise ops. The two pair ops come after the AccOp codes (below), so
// that every code handed out so far keeps its value.
enum PeerOp : int {
  kPrSum = 0, kPrProd, kPrMax, kPrMin, kPrLand, kPrLor, kPrLxor, kPrBand, kPrBor, kPrBxor, kPrOps,
  kPrMaxloc = 12, kPrMinloc = 13
};
// kPrDtypes counts the seven scalar types. A pair layout of MAXLOC / MINLOC is one more element
// type, and n then counts pairs: kPrPair + t is (value, index) interleaved in scalar type t
// (2INT is kPrPair + kPrI32); the struct pairs are laid out as MPI lays them out:
// FLOAT_INT f32 at 0, i32 at 4, extent 8; DOUBLE_INT f64 at 0, i32 at 8, extent 16; LONG_INT i64
// at 0, i32 at 8, extent 16. Pointers of a pair type need the alignment of its largest member only.
enum PeerDtype : int {
  kPrF32 = 0, kPrBf16, kPrF16, kPrF64, kPrI32, kPrI64, kPrU8, kPrDtypes,
  kPrPair = 16, kPrFloatInt = 24, kPrDoubleInt = 25, kPrLongInt = 26
};
constexpr int kPeerMax = 8;
// dst[j][i] = src[0][i] (op) src[1][i] (op) ... (op) src[ns-1][i], i < n, for every j < nd:
// a left fold in the order given; 1 <= ns <= 8, 1 <= nd <= 8; dev < 0 -> host twin.
// bf16 / fp16 SUM and PROD accumulate in fp32 and round to nearest-even once at the store;
// MAX / MIN propagate NaN; LAND / LOR / LXOR: non-zero is true, result 0 or 1 in the dtype;
// BAND / BOR / BXOR: integer dtypes only. MAXLOC / MINLOC: the pair types only, and nothing else
// on them; the result is one of the operand pairs, every byte of it (peer_ops.h has the rule).
// dst[j] may be src[j] (in place); nothing else may
// alias. The kernel holds no cross-rank synchronisation: visibility rests on its boundaries.
bool peer_reduce_supported(int op, int dtype);
int peer_dtype_size(int dtype);   // bytes of one element: the extent of a pair
int peer_dtype_align(int dtype);  // the alignment a pointer needs: that of the largest member
bool peer_dtype_is_pair(int dtype);
void peer_reduce(int dev, hipStream_t s, int op, int dtype, const std::vector<uintptr_t>& srcs,
                 const std::vector<uintptr_t>& dsts, int64_t n);

// ---- the kernels of the window collectives (peer_coll.hip; peer_fold: allreduce.hip) ---
// One launch on `s` each, or the host twin for dev < 0. Element types, ops, widening, rounding
// and combine are peer_reduce's: the same operands give the same bits. No pointer of a call
// needs to share its offset within 16 B with another (element alignment is all that is asked).
// max_blocks: 0 = the production cap of the grid, > 0 = at most that many blocks (tests).
// No cross-rank synchronisation inside; allocates and synchronises nothing.
//
// peer_gather: up to 8 independent byte segments, dst[g][0..bytes[g]) = src[g][0..bytes[g]), at
// any alignment of either side. Zero-length segments and segments with src == dst are dropped;
// destinations are disjoint from each other and from every source.
void peer_gather(int dev, hipStream_t s, const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts,
                 const std::vector<int64_t>& bytes, int max_blocks = 0);
// peer_fold: dst[i] = src[0][i] (op) ... (op) src[ns-1][i], i < n, 1 <= ns <= 8, one destination
// that aliases no source.
void peer_fold(int dev, hipStream_t s, int op, int dtype, const std::vector<uintptr_t>& srcs, uintptr_t dst, int64_t n,
               int max_blocks = 0);
// peer_scan: inclusive dst[j][i] = src[0][i] (op) ... (op) src[j][i] for every j < ns; exclusive
// dst[j][i] = src[0][i] (op) ... (op) src[j-1][i] for 1 <= j < ns, dst[0] never written (it may be
// 0). The accumulator stays wide across the chain: a 16-bit float prefix is rounded once.
// dst[j] may be src[j] (in place); nothing else may alias.
void peer_scan(int dev, hipStream_t s, int op, int dtype, bool exclusive, const std::vector<uintptr_t>& srcs,
               const std::vector<uintptr_t>& dsts, int64_t n, int max_blocks = 0);

// ---- derived-datatype pack / unpack (type_copy.hip) ------------------------------------
// dir 0: gather the strided layout at `strided` into the contiguous stream at `packed`; dir 1:
// scatter the stream into the layout. The layout is up to three `loops` (count, byte stride),
// outermost first, around R runs: table = int64 [offs[R] | prefix[R + 1]] (device memory, host
// when dev < 0), L = the common run length or 0, per = prefix[R] = the packed bytes of one
// innermost iteration (R * L when L != 0). table == 0 with R == 1, L != 0: one run at offset 0.
// Packed order: loops outermost to innermost, runs in table order, ascending bytes. unit (a power
// of two <= 16) divides every offset, length, stride (of a loop with count > 1) and both
// addresses: bytes moved per lane and access. max_blocks > 0 lowers the grid cap; wide forces the
// 64-bit index arithmetic that a packed stream of 4 GiB or more selects by itself. The layout is
// trusted: the caller has checked its span against the buffers. Allocates and synchronises
// nothing. Overlapping runs in a scatter leave one writer's bytes.
void type_copy(int dev, hipStream_t s, int dir, uintptr_t strided, uintptr_t packed,
               const std::vector<std::array<int64_t, 2>>& loops, uintptr_t table, int64_t R, int64_t L, int64_t per,
               int unit, int max_blocks = 0, bool wide = false);

// ---- layout-to-layout gather of up to 8 segments (peer_plan.hip) --------------------------
// The kernel of the irregular window collectives (Window::pull_plan). A side is a base address
// plus a layout exactly as type_copy takes it (loops, table, R, L, per; a contiguous side is the
// one-run layout: no loops, no table, R = 1, L = per = its bytes). For every packed byte q of
// every segment g: dst_g[off_dst(q)] = src_g[off_src(q)], packed order as in type_copy. `unit` (a
// power of two <= 16) divides every offset, length, stride and the base address of BOTH sides of
// its segment: one lane moves one unit per access. One launch on `s` for all segments together
// (blocks find their segment in a prefix table of tile counts), or the host twin for dev < 0.
// std::invalid_argument, before any launch: more than 8 segments, sides of unequal packed size,
// and what type_copy refuses of either side. Dropped: zero-length segments and segments whose two
// sides are the same address and layout. Destinations are disjoint from each other and from
// every source. Run tables up to 1,024 runs are staged in LDS, longer ones read from global
// memory. max_blocks and wide as in type_copy (64-bit indices by themselves when a segment packs
// 4 GiB or more). The layouts are trusted. Allocates and synchronises nothing; no atomics, no
// cross-rank communication. peer_plan_check makes the checks alone.
struct PlanSide {
  uintptr_t base;
  std::vector<std::array<int64_t, 2>> loops;
  uintptr_t table;
  int64_t R, L, per;
};
struct PlanSegment {
  PlanSide src, dst;
  int unit;
};
void peer_plan_check(const std::vector<PlanSegment>& segs);
void peer_plan_gather(int dev, hipStream_t s, const std::vector<PlanSegment>& segs, int max_blocks = 0,
                      bool wide = false);

// ---- one-sided accumulate on a derived-datatype layout (type_acc.hip) --------------------
// For every element e of the layout (type_copy's: loops, table, R, L, per, unit; the same run
// modes, index widths, max_blocks and wide), in one launch on `s`, or the host twin for dev < 0:
//     old = strided[e];  strided[e] = comb(op, old, packed[e]);  fetch[e] = old   (fetch != 0)
// a = the target element, b = the origin element, comb / widen / narrow those of peer_reduce:
// the same operands give the same bits as the all-reduce. op: a PeerOp, kAccReplace (store the
// origin element) or kAccNoOp (store nothing: only meaningful with a fetch stream; packed may
// be 0). dtype: a PeerDtype. `packed` and `fetch` are contiguous streams of the layout's packed
// size. One item is `unit` bytes = unit / sizeof(element) elements: std::invalid_argument when
// unit < sizeof(element) (a pair type's element is the whole pair), for an unsupported (op, dtype)
// (type_accumulate_supported: what peer_reduce_supported takes, REPLACE and NO_OP on the seven
// scalar types) and for what type_copy refuses,
// before any launch. No atomics: the caller holds the target's exclusive lock. The layout is
// trusted; overlapping target runs are erroneous (as for MPI_Accumulate) and undefined here.
// Allocates and synchronises nothing.
enum AccOp : int { kAccReplace = kPrOps, kAccNoOp, kAccOps };
bool type_accumulate_supported(int op, int dtype);
void type_accumulate(int dev, hipStream_t s, int op, int dtype, uintptr_t strided, uintptr_t packed, uintptr_t fetch,
                     const std::vector<std::array<int64_t, 2>>& loops, uintptr_t table, int64_t R, int64_t L,
                     int64_t per, int unit, int max_blocks = 0, bool wide = false);

}  // namespace mpit
