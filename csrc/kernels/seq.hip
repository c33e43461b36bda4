// Forward-only sentence encoder and GESD scoring of the BiCNN tower (ops/seq.py; the reference's
// LookupTable -> Linear -> Tanh -> TemporalConvolution -> Max -> ReLU -> Normalize tower and its
// similarity, BiCNN/bicnn.lua:30-121), fp32, for the encodes that run without autograd (the
// negative-sampling scan and the tester). Three streaming kernels around the fp32 gemm_nt:
//   seq_hidden_windows: tok -> the im2col rows of the temporal convolution,
//       out[(b,t)][j*H + i] = tanh(bh[i] + sum_d E[tok[b][t+j]][d] * Wh[i][d]); each token's hidden
//       vector is computed once (embedding rows staged in LDS, nothing else leaves the chip) and
//       stored to its up-to-k places, missing taps and the pad columns are written as zeros;
//   seq_max_norm: masked max over time of the GEMM output + bias + ReLU (phase 1, F / 256 blocks
//       per sentence), then the L2 normalisation (phase 2, one block per sentence);
//   gesd_gather: 1 / (1 + |q - c|) * sigmoid(q . c + 1) of gathered row pairs, one wave per pair,
//       both reductions in one read of the two rows.
// Every reduction runs in an order fixed by the row length alone (never by the batch, the
// sentence length or the grid), so a sentence's encoding and a pair's score are the same bits in
// any batch. No atomics, no cross-block communication.
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>

#include "ew.h"
#include "kernels.h"

namespace mpit {
namespace {

constexpr int kSeqThreads = 256;
constexpr int kSeqTok = 16;  // tokens per block of seq_hidden_windows

// One block: kSeqTok consecutive tokens n = b*T + t. Their embedding rows go to LDS; thread i
// (strided over H) walks Wh[i][:] once and keeps one accumulator per token (d ascending, one
// fmaf per term, the bias added last: a token's value does not depend on its neighbours).
__global__ __launch_bounds__(kSeqThreads) void seq_hidden_windows_kernel(
    const int64_t* __restrict__ tok, int64_t ntok, int T, const float* __restrict__ E, int D,
    const float* __restrict__ Wh, const float* __restrict__ bh, int H, int k, float* __restrict__ out, int Kp) {
  extern __shared__ float emb[];  // [kSeqTok][D]
  const int64_t n0 = int64_t(blockIdx.x) * kSeqTok;
  const int cnt = ntok - n0 < kSeqTok ? int(ntok - n0) : kSeqTok;
  for (int e = threadIdx.x; e < kSeqTok * D; e += kSeqThreads) {
    const int p = e / D, d = e - p * D;
    emb[e] = p < cnt ? E[tok[n0 + p] * D + d] : 0.f;  // (slots past the last token: zeros, never stored)
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += kSeqThreads) {
    float acc[kSeqTok];
#pragma unroll
    for (int p = 0; p < kSeqTok; ++p) acc[p] = 0.f;
    const float* w = Wh + int64_t(i) * D;
    for (int d = 0; d < D; ++d) {
      const float wv = w[d];
#pragma unroll
      for (int p = 0; p < kSeqTok; ++p) acc[p] = fmaf(emb[p * D + d], wv, acc[p]);
    }
    const float bias = bh ? bh[i] : 0.f;
#pragma unroll
    for (int p = 0; p < kSeqTok; ++p) {
      if (p >= cnt) continue;
      const float h = tanhf(bias + acc[p]);
      const int64_t n = n0 + p;
      const int t = int(n % T);
      // tap j of row (b, t - j); the rows of one sentence are consecutive
      for (int j = 0; j < k && j <= t; ++j) out[(n - j) * Kp + int64_t(j) * H + i] = h;
      // this row's missing taps (t + j >= T)
      for (int j = max(1, T - t); j < k; ++j) out[n * Kp + int64_t(j) * H + i] = 0.f;
    }
  }
  // pad columns k*H .. Kp-1 of this block's rows
  const int kh = k * H, padw = Kp - kh;
  for (int e = threadIdx.x; e < cnt * padw; e += kSeqThreads) {
    const int p = e / padw, c = e - p * padw;
    out[(n0 + p) * Kp + kh + c] = 0.f;
  }
}

// phase 1: m[b][f] = max(0, bias[f] + max over valid t of c[(b,t)][f]) (0 without a valid window).
// Window (b,t) is valid iff t <= T-k and tok[b][t+k-1] != pad_idx. grid (ceil(F/256), B).
__global__ __launch_bounds__(kSeqThreads) void seq_max_kernel(const float* __restrict__ c, int64_t ldc,
                                                              const int64_t* __restrict__ tok, int T, int k,
                                                              int64_t pad_idx, const float* __restrict__ bias, int F,
                                                              float* __restrict__ out) {
  const int f = blockIdx.x * kSeqThreads + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (f >= F) return;
  const int64_t* tb = tok + b * T;
  const float* cb = c + b * T * ldc + f;
  float m = -INFINITY;
  bool any = false;
  for (int t = 0; t + k <= T; ++t) {
    if (tb[t + k - 1] == pad_idx) continue;  // (block-uniform: no divergence)
    m = fmaxf(m, cb[t * ldc]);
    any = true;
  }
  float v = 0.f;
  if (any) {
    v = m + (bias ? bias[f] : 0.f);
    v = v > 0.f ? v : 0.f;  // (+0.0 for -0.0 too)
  }
  out[b * F + f] = v;
}

// phase 2: out[b][:] /= max(sqrt(sum_f out[b][f]^2), eps). One block per sentence; the sum runs
// thread-strided, then the wave butterfly, then the waves in order: fixed by F alone.
__global__ __launch_bounds__(kSeqThreads) void seq_norm_kernel(float* __restrict__ out, int F, float eps) {
  __shared__ float red[kSeqThreads / 64];
  float* o = out + int64_t(blockIdx.x) * F;
  float s = 0.f;
  for (int f = threadIdx.x; f < F; f += kSeqThreads) s = fmaf(o[f], o[f], s);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  float tot = red[0];
  for (int w = 1; w < kSeqThreads / 64; ++w) tot += red[w];
  const float den = fmaxf(__fsqrt_rn(tot), eps);
  for (int f = threadIdx.x; f < F; f += kSeqThreads) o[f] = __fdiv_rn(o[f], den);
}

// One wave per (r, c) pair: lane l sums d = l, l + 64, ... of both reductions, then the butterfly.
__global__ __launch_bounds__(kSeqThreads) void gesd_gather_kernel(const float* __restrict__ q,
                                                                  const float* __restrict__ cand,
                                                                  const int64_t* __restrict__ idx, int64_t npairs,
                                                                  int w, int D, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = int64_t(blockIdx.x) * (kSeqThreads / 64) + (threadIdx.x >> 6);
  if (pair >= npairs) return;
  const float* a = q + (pair / w) * D;
  const float* b = cand + idx[pair] * D;
  float ss = 0.f, dot = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float x = a[d], y = b[d], e = x - y;
    ss = fmaf(e, e, ss);
    dot = fmaf(x, y, dot);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ss += __shfl_xor(ss, o);
    dot += __shfl_xor(dot, o);
  }
  if (lane == 0)
    out[pair] = __fdiv_rn(1.f, 1.f + __fsqrt_rn(ss)) * __fdiv_rn(1.f, 1.f + expf(-(dot + 1.f)));
}

void need_dev(int dev, const char* what) {
  if (dev < 0) throw std::invalid_argument(std::string(what) + ": device tensors only");
}

}  // namespace

void seq_hidden_windows(int dev, hipStream_t s, uintptr_t tok, int64_t B, int T, uintptr_t E, int D, uintptr_t Wh,
                        uintptr_t bh, int H, int k, uintptr_t out, int Kp) {
  need_dev(dev, "seq_hidden_windows");
  if (B <= 0 || T <= 0 || D <= 0 || H <= 0 || k <= 0 || int64_t(k) * H > Kp)
    throw std::invalid_argument("seq_hidden_windows: bad shape");
  const size_t lds = size_t(kSeqTok) * D * sizeof(float);
  if (lds > 48 * 1024) throw std::invalid_argument("seq_hidden_windows: embedding dim too large");
  const int64_t ntok = B * T, nblk = (ntok + kSeqTok - 1) / kSeqTok;
  if (nblk > INT32_MAX) throw std::invalid_argument("seq_hidden_windows: too many tokens");
  if (!tok || !E || !Wh || !out) throw std::invalid_argument("seq_hidden_windows: null pointer");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  hipLaunchKernelGGL(seq_hidden_windows_kernel, dim3(unsigned(nblk)), dim3(kSeqThreads), lds, s,
                     reinterpret_cast<const int64_t*>(tok), ntok, T, reinterpret_cast<const float*>(E), D,
                     reinterpret_cast<const float*>(Wh), reinterpret_cast<const float*>(bh), H, k,
                     reinterpret_cast<float*>(out), Kp);
  hip_check(hipGetLastError(), "seq_hidden_windows launch");
}

void seq_max_norm(int dev, hipStream_t s, uintptr_t c, int64_t ldc, uintptr_t tok, int64_t B, int T, int k,
                  int64_t pad_idx, uintptr_t bias, int F, float eps, uintptr_t out) {
  need_dev(dev, "seq_max_norm");
  if (B <= 0 || T <= 0 || k <= 0 || F <= 0 || ldc < F) throw std::invalid_argument("seq_max_norm: bad shape");
  if (B > 65535) throw std::invalid_argument("seq_max_norm: more than 65535 sentences");
  if (!c || !tok || !out) throw std::invalid_argument("seq_max_norm: null pointer");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  const dim3 g1{unsigned((F + kSeqThreads - 1) / kSeqThreads), unsigned(B)};
  hipLaunchKernelGGL(seq_max_kernel, g1, dim3(kSeqThreads), 0, s, reinterpret_cast<const float*>(c), ldc,
                     reinterpret_cast<const int64_t*>(tok), T, k, pad_idx, reinterpret_cast<const float*>(bias), F,
                     reinterpret_cast<float*>(out));
  hip_check(hipGetLastError(), "seq_max launch");
  hipLaunchKernelGGL(seq_norm_kernel, dim3(unsigned(B)), dim3(kSeqThreads), 0, s, reinterpret_cast<float*>(out), F,
                     eps);
  hip_check(hipGetLastError(), "seq_norm launch");
}

void gesd_gather(int dev, hipStream_t s, uintptr_t q, uintptr_t cand, uintptr_t idx, int64_t n, int w, int D,
                 uintptr_t out) {
  need_dev(dev, "gesd_gather");
  if (n <= 0 || w <= 0 || D <= 0) throw std::invalid_argument("gesd_gather: bad shape");
  if (!q || !cand || !idx || !out) throw std::invalid_argument("gesd_gather: null pointer");
  const int64_t npairs = n * w, nblk = (npairs + kSeqThreads / 64 - 1) / (kSeqThreads / 64);
  if (nblk > INT32_MAX) throw std::invalid_argument("gesd_gather: too many pairs");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  hipLaunchKernelGGL(gesd_gather_kernel, dim3(unsigned(nblk)), dim3(kSeqThreads), 0, s,
                     reinterpret_cast<const float*>(q), reinterpret_cast<const float*>(cand),
                     reinterpret_cast<const int64_t*>(idx), npairs, w, D, reinterpret_cast<float*>(out));
  hip_check(hipGetLastError(), "gesd_gather launch");
}

}  // namespace mpit
