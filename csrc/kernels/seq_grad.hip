// Per-example gradients of the BiCNN margin loss (ops/seq.py per_example_grads; the parity rule
// of models/bicnn.py parity_grad_), fp32, without autograd. The forward half is the kernels of
// seq.hip bit for bit (the max / norm kernels below repeat their operation order and also write
// the arg-max and the clamped norm); the backward uses the structure a generic vmap cannot: one
// arg-max row per (sentence, filter), three sentences per example, at most 3T embedding rows.
//   seq_max_norm_arg:   y[S][F] (the encoder's bits), arg[S][F] (first window attaining the max, -1
//                       without a valid window or with a ReLU output of 0), den[S];
//   gesd_pair_bwd:      one block per example: the two GESD scores (gesd_gather's bits), the hinge
//                       value and the gradient of the three encodings;
//   seq_norm_max_bwd:   dm = gradient of the max (through the normalisation and the ReLU) and the
//                       whole of dc[S*T][Fp]: dm at row (s, arg), zero everywhere else;
//   (dwin = dc . Wp: the fp32 gemm_nt against the transposed packed weight)
//   seq_conv_wgrad_pe:  per-example convolution weight / bias gradients from the three arg-max
//                       rows of a filter (T times less work than a dense weight-gradient GEMM);
//   seq_hidden_bwd:     da = (1 - h^2) * (the window gradient folded back onto its tokens) and
//                       de = Wh^T da per token;
//   seq_hidden_wgrad_pe: dWh[k] = sum da (x) E[tok], dbh[k] = sum da over the example's tokens;
//   seq_embed_grad_pe:  the example's touched embedding rows, each written once by the first
//                       occurrence of its word.
// Sentence s of S = 3n belongs to example s % n (q, a_pos, a_neg stacked). Every reduction runs in
// an order fixed by F, H, D, k and the example's own tokens (q, a_pos, a_neg, ascending t): a row
// of g never depends on n, on the padding or on the grid. No atomics, no cross-block traffic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>
#include <string>

#include "ew.h"
#include "kernels.h"

namespace mpit {
namespace {

constexpr int kThreads = 256;
constexpr int kTok = 16;     // tokens per block of seq_hidden_bwd
constexpr int kDcRows = 8;   // rows of dc per block of seq_norm_max_bwd
constexpr int kWgF = 4;      // filters per block of seq_conv_wgrad_pe

// seq_max_kernel of seq.hip (same comparisons, same bias add) + the first t attaining the max.
__global__ __launch_bounds__(kThreads) void seq_max_arg_kernel(const float* __restrict__ c, int64_t ldc,
                                                               const int64_t* __restrict__ tok, int T, int k,
                                                               int64_t pad_idx, const float* __restrict__ bias, int F,
                                                               float* __restrict__ out, int* __restrict__ arg) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (f >= F) return;
  const int64_t* tb = tok + b * T;
  const float* cb = c + b * T * ldc + f;
  float m = -INFINITY;
  int at = -1;
  bool any = false;
  for (int t = 0; t + k <= T; ++t) {
    if (tb[t + k - 1] == pad_idx) continue;
    const float v = cb[t * ldc];
    if (!any || v > m) at = t;
    m = fmaxf(m, v);
    any = true;
  }
  float v = 0.f;
  if (any) {
    v = m + (bias ? bias[f] : 0.f);
    v = v > 0.f ? v : 0.f;
  }
  out[b * F + f] = v;
  arg[b * F + f] = v > 0.f ? at : -1;
}

// seq_norm_kernel of seq.hip + den[b].
__global__ __launch_bounds__(kThreads) void seq_norm_den_kernel(float* __restrict__ out, int F, float eps,
                                                                float* __restrict__ den_out) {
  __shared__ float red[kThreads / 64];
  float* o = out + int64_t(blockIdx.x) * F;
  float s = 0.f;
  for (int f = threadIdx.x; f < F; f += kThreads) s = fmaf(o[f], o[f], s);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  float tot = red[0];
  for (int w = 1; w < kThreads / 64; ++w) tot += red[w];
  const float den = fmaxf(__fsqrt_rn(tot), eps);
  for (int f = threadIdx.x; f < F; f += kThreads) o[f] = __fdiv_rn(o[f], den);
  if (threadIdx.x == 0) den_out[blockIdx.x] = den;
}

// One block per example k. Waves 0 and 1 run gesd_gather_kernel's two reductions for the pairs
// (q, a_pos) and (q, a_neg); then every thread forms the scores and walks its columns.
__global__ __launch_bounds__(kThreads) void gesd_pair_bwd_kernel(const float* __restrict__ y, int64_t n, int F,
                                                                 float margin, float* __restrict__ err,
                                                                 float* __restrict__ sc, float* __restrict__ gy) {
  __shared__ float red[4];  // ss_pos, dot_pos, ss_neg, dot_neg
  const int64_t ex = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* q = y + ex * F;
  const float* ap = y + (n + ex) * F;
  const float* an = y + (2 * n + ex) * F;
  if (wave < 2) {
    const float* b = wave == 0 ? ap : an;
    float ss = 0.f, dot = 0.f;
    for (int d = lane; d < F; d += 64) {
      const float x = q[d], z = b[d], e = x - z;
      ss = fmaf(e, e, ss);
      dot = fmaf(x, z, dot);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ss += __shfl_xor(ss, o);
      dot += __shfl_xor(dot, o);
    }
    if (lane == 0) {
      red[2 * wave] = ss;
      red[2 * wave + 1] = dot;
    }
  }
  __syncthreads();
  const float Lp = __fsqrt_rn(red[0]), Ln = __fsqrt_rn(red[2]);
  const float Ap = __fdiv_rn(1.f, 1.f + Lp), An = __fdiv_rn(1.f, 1.f + Ln);
  const float Bp = __fdiv_rn(1.f, 1.f + expf(-(red[1] + 1.f))), Bn = __fdiv_rn(1.f, 1.f + expf(-(red[3] + 1.f)));
  // (rounded products and sums, never contracted: sp and sn are gesd_gather's bits)
  const float sp = __fmul_rn(Ap, Bp), sn = __fmul_rn(An, Bn);
  float e = __fadd_rn(__fsub_rn(margin, sp), sn);
  e = e > 0.f ? e : 0.f;
  if (threadIdx.x == 0) {
    err[ex] = e;
    sc[ex] = sp;
    sc[n + ex] = sn;
  }
  float* gq = gy + ex * F;
  float* gp = gy + (n + ex) * F;
  float* gn = gy + (2 * n + ex) * F;
  if (!(e > 0.f)) {
    for (int f = threadIdx.x; f < F; f += kThreads) gq[f] = gp[f] = gn[f] = 0.f;
    return;
  }
  // ds/da = -A^2 B (a - b) / L + A B (1 - B) b, ds/db = +A^2 B (a - b) / L + A B (1 - B) a;
  // the distance term is 0 where L == 0. loss = margin - sp + sn.
  const float dp = Lp > 0.f ? Ap * Ap * Bp / Lp : 0.f, dn = Ln > 0.f ? An * An * Bn / Ln : 0.f;
  const float tp = Ap * Bp * (1.f - Bp), tn = An * Bn * (1.f - Bn);
  for (int f = threadIdx.x; f < F; f += kThreads) {
    const float a = q[f], p = ap[f], ng = an[f];
    const float dsp_da = tp * p - dp * (a - p), dsp_db = tp * a + dp * (a - p);
    const float dsn_da = tn * ng - dn * (a - ng), dsn_db = tn * a + dn * (a - ng);
    gq[f] = dsn_da - dsp_da;
    gp[f] = -dsp_db;
    gn[f] = dsn_db;
  }
}

// grid (S, ceil(T / kDcRows)). Every block forms r = sum_f gy * y of its sentence in
// seq_norm_kernel's order, then dm for the columns of each thread (4 consecutive ones) and
// stores its kDcRows rows of dc as float4 (Fp % 4 == 0, rows 16-byte aligned). Block y == 0
// also writes dm[s][:].
__global__ __launch_bounds__(kThreads) void seq_norm_max_bwd_kernel(const float* __restrict__ gy,
                                                                    const float* __restrict__ y,
                                                                    const int* __restrict__ arg,
                                                                    const float* __restrict__ den, int T, int F,
                                                                    int Fp, float eps, float* __restrict__ dm,
                                                                    float* __restrict__ dc) {
  __shared__ float red[kThreads / 64];
  const int64_t s = blockIdx.x;
  const float* g = gy + s * F;
  const float* ys = y + s * F;
  const int* as = arg + s * F;
  float r = 0.f;
  for (int f = threadIdx.x; f < F; f += kThreads) r = fmaf(g[f], ys[f], r);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) r += __shfl_xor(r, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
  __syncthreads();
  float tot = red[0];
  for (int w = 1; w < kThreads / 64; ++w) tot += red[w];
  const float dn = den[s];
  if (!(dn > eps)) tot = 0.f;  // the clamped norm passes no gradient through the norm itself
  const int t0 = blockIdx.y * kDcRows, t1 = min(T, t0 + kDcRows);
  for (int f0 = threadIdx.x * 4; f0 < Fp; f0 += kThreads * 4) {
    float v[4];
    int a[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = f0 + e;
      a[e] = f < F ? as[f] : -1;
      v[e] = a[e] >= 0 ? __fdiv_rn(g[f] - ys[f] * tot, dn) : 0.f;
      if (blockIdx.y == 0 && f < F) dm[s * F + f] = v[e];
    }
    for (int t = t0; t < t1; ++t) {
      float4 o;
      o.x = a[0] == t ? v[0] : 0.f;
      o.y = a[1] == t ? v[1] : 0.f;
      o.z = a[2] == t ? v[2] : 0.f;
      o.w = a[3] == t ? v[3] : 0.f;
      *reinterpret_cast<float4*>(dc + (s * T + t) * Fp + f0) = o;
    }
  }
}

// grid (ceil(F / kWgF), n). Output element o = i * k + j of filter f (the [F][H][k] weight):
// sum over s = ex, n + ex, 2n + ex of dm[s][f] * win[(s, arg[s][f])][j * H + i].
__global__ __launch_bounds__(kThreads) void seq_conv_wgrad_pe_kernel(const float* __restrict__ dm,
                                                                     const int* __restrict__ arg,
                                                                     const float* __restrict__ win, int64_t n, int T,
                                                                     int F, int H, int k, int Kp,
                                                                     float* __restrict__ g, int64_t ldg, int64_t offW,
                                                                     int64_t offB) {
  const int64_t ex = blockIdx.y;
  const int hk = H * k;
  float* gw = g + ex * ldg + offW;
  for (int ff = 0; ff < kWgF; ++ff) {
    const int f = blockIdx.x * kWgF + ff;
    if (f >= F) return;
    float d[3];
    const float* row[3];
    bool on[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int64_t s = u * n + ex;
      const int a = arg[s * F + f];
      on[u] = a >= 0;
      d[u] = dm[s * F + f];
      row[u] = win + (s * T + (on[u] ? a : 0)) * Kp;
    }
    for (int o = threadIdx.x; o < hk; o += kThreads) {
      const int i = o / k, j = o - i * k;
      const int col = j * H + i;
      float acc = 0.f;
#pragma unroll
      for (int u = 0; u < 3; ++u)
        if (on[u]) acc = fmaf(d[u], row[u][col], acc);
      gw[int64_t(f) * hk + o] = acc;
    }
    if (threadIdx.x == 0 && offB >= 0) g[ex * ldg + offB + f] = (d[0] + d[1]) + d[2];
  }
}

// One block: kTok consecutive tokens r = s*T + t. Phase 1: da[r][i] = (1 - h^2) * sum over the
// taps j < k, j <= t of dwin[r - j][j*H + i] (j ascending), h = win[r][i]; to LDS and to HBM.
// Phase 2: de[r][d] = sum_i Wh[i][d] * da[r][i] (i ascending, one fmaf per term).
__global__ __launch_bounds__(kThreads) void seq_hidden_bwd_kernel(const float* __restrict__ dwin, int64_t ldw,
                                                                  const float* __restrict__ win, int Kp, int64_t ntok,
                                                                  int T, int H, int k, const float* __restrict__ Wh,
                                                                  int D, float* __restrict__ da,
                                                                  float* __restrict__ de) {
  extern __shared__ float lda_[];  // [kTok][H]
  const int64_t r0 = int64_t(blockIdx.x) * kTok;
  const int cnt = ntok - r0 < kTok ? int(ntok - r0) : kTok;
  for (int e = threadIdx.x; e < kTok * H; e += kThreads) {
    const int p = e / H, i = e - p * H;
    float v = 0.f;
    if (p < cnt) {
      const int64_t r = r0 + p;
      const int t = int(r % T);
      float acc = 0.f;
      for (int j = 0; j < k && j <= t; ++j) acc += dwin[(r - j) * ldw + int64_t(j) * H + i];
      const float h = win[r * Kp + i];
      v = (1.f - h * h) * acc;
      da[r * H + i] = v;
    }
    lda_[e] = v;
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += kThreads) {
    float acc[kTok];
#pragma unroll
    for (int p = 0; p < kTok; ++p) acc[p] = 0.f;
    for (int i = 0; i < H; ++i) {
      const float w = Wh[int64_t(i) * D + d];
#pragma unroll
      for (int p = 0; p < kTok; ++p) acc[p] = fmaf(lda_[p * H + i], w, acc[p]);
    }
#pragma unroll
    for (int p = 0; p < kTok; ++p)
      if (p < cnt) de[(r0 + p) * D + d] = acc[p];
  }
}

// grid (ceil(H * D / 256), n): thread -> element (i, d) of dWh[ex]; the example's 3T tokens in
// the order q, a_pos, a_neg with ascending t. The threads with d == 0 also write dbh[ex][i].
__global__ __launch_bounds__(kThreads) void seq_hidden_wgrad_pe_kernel(const float* __restrict__ da,
                                                                       const int64_t* __restrict__ tok,
                                                                       const float* __restrict__ E, int64_t n, int T,
                                                                       int H, int D, float* __restrict__ g,
                                                                       int64_t ldg, int64_t offWh, int64_t offBh) {
  const int64_t ex = blockIdx.y;
  const int o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= H * D) return;
  const int i = o / D, d = o - i * D;
  float acc = 0.f, sb = 0.f;
  for (int u = 0; u < 3; ++u) {
    const int64_t r0 = (u * n + ex) * T;
    for (int t = 0; t < T; ++t) {
      const float a = da[(r0 + t) * H + i];
      acc = fmaf(a, E[tok[r0 + t] * D + d], acc);
      sb += a;
    }
  }
  g[ex * ldg + offWh + o] = acc;
  if (d == 0 && offBh >= 0) g[ex * ldg + offBh + i] = sb;
}

// grid (ceil(3T / 4), n): one wave per token position p of the example (ids staged in LDS). The
// first occurrence of a word sums de over its later occurrences (in token order) and writes the
// row; later occurrences and pad_idx write nothing.
__global__ __launch_bounds__(kThreads) void seq_embed_grad_pe_kernel(const float* __restrict__ de,
                                                                     const int64_t* __restrict__ tok, int64_t n,
                                                                     int T, int D, int64_t V, int64_t pad_idx,
                                                                     float* __restrict__ g, int64_t ldg,
                                                                     int64_t offE) {
  extern __shared__ int64_t ids[];  // [3T]
  const int64_t ex = blockIdx.y;
  const int np = 3 * T;
  for (int p = threadIdx.x; p < np; p += kThreads) ids[p] = tok[((p / T) * n + ex) * T + (p % T)];
  __syncthreads();
  const int p = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (p >= np) return;
  const int64_t id = ids[p];
  if (id == pad_idx || id < 0 || id >= V) return;  // (an id outside the table never becomes a store)
  for (int e = 0; e < p; ++e)
    if (ids[e] == id) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  for (int d = lane; d < D; d += 64) {
    float acc = de[(((p / T) * n + ex) * T + (p % T)) * D + d];
    for (int e = p + 1; e < np; ++e)
      if (ids[e] == id) acc += de[(((e / T) * n + ex) * T + (e % T)) * D + d];
    g[ex * ldg + offE + id * D + d] = acc;
  }
}

void need_dev(int dev, const char* what) {
  if (dev < 0) throw std::invalid_argument(std::string(what) + ": device tensors only");
}

template <class T>
T* P(uintptr_t p) {
  return reinterpret_cast<T*>(p);
}

}  // namespace

void seq_max_norm_arg(int dev, hipStream_t s, uintptr_t c, int64_t ldc, uintptr_t tok, int64_t B, int T, int k,
                      int64_t pad_idx, uintptr_t bias, int F, float eps, uintptr_t out, uintptr_t arg, uintptr_t den) {
  need_dev(dev, "seq_max_norm_arg");
  if (B <= 0 || T <= 0 || k <= 0 || F <= 0 || ldc < F) throw std::invalid_argument("seq_max_norm_arg: bad shape");
  if (B > 65535) throw std::invalid_argument("seq_max_norm_arg: more than 65535 sentences");
  if (!c || !tok || !out || !arg || !den) throw std::invalid_argument("seq_max_norm_arg: null pointer");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  const dim3 g1{unsigned((F + kThreads - 1) / kThreads), unsigned(B)};
  hipLaunchKernelGGL(seq_max_arg_kernel, g1, dim3(kThreads), 0, s, P<const float>(c), ldc, P<const int64_t>(tok), T,
                     k, pad_idx, P<const float>(bias), F, P<float>(out), P<int>(arg));
  hip_check(hipGetLastError(), "seq_max_arg launch");
  hipLaunchKernelGGL(seq_norm_den_kernel, dim3(unsigned(B)), dim3(kThreads), 0, s, P<float>(out), F, eps,
                     P<float>(den));
  hip_check(hipGetLastError(), "seq_norm_den launch");
}

void gesd_pair_bwd(int dev, hipStream_t s, uintptr_t y, int64_t n, int F, float margin, uintptr_t err, uintptr_t sc,
                   uintptr_t gy) {
  need_dev(dev, "gesd_pair_bwd");
  if (n <= 0 || F <= 0 || n > INT32_MAX / 3) throw std::invalid_argument("gesd_pair_bwd: bad shape");
  if (!y || !err || !sc || !gy) throw std::invalid_argument("gesd_pair_bwd: null pointer");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  hipLaunchKernelGGL(gesd_pair_bwd_kernel, dim3(unsigned(n)), dim3(kThreads), 0, s, P<const float>(y), n, F, margin,
                     P<float>(err), P<float>(sc), P<float>(gy));
  hip_check(hipGetLastError(), "gesd_pair_bwd launch");
}

void seq_norm_max_bwd(int dev, hipStream_t s, uintptr_t gy, uintptr_t y, uintptr_t arg, uintptr_t den, int64_t S, int T,
                      int F, int Fp, float eps, uintptr_t dm, uintptr_t dc) {
  need_dev(dev, "seq_norm_max_bwd");
  if (S <= 0 || T <= 0 || F <= 0 || Fp < F || Fp % 4) throw std::invalid_argument("seq_norm_max_bwd: bad shape");
  const int64_t ny = (int64_t(T) + kDcRows - 1) / kDcRows;
  if (S > INT32_MAX || ny > 65535) throw std::invalid_argument("seq_norm_max_bwd: too many sentences or tokens");
  if (!gy || !y || !arg || !den || !dm || !dc) throw std::invalid_argument("seq_norm_max_bwd: null pointer");
  if (dc % 16) throw std::invalid_argument("seq_norm_max_bwd: dc must be 16-byte aligned");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  hipLaunchKernelGGL(seq_norm_max_bwd_kernel, dim3(unsigned(S), unsigned(ny)), dim3(kThreads), 0, s,
                     P<const float>(gy), P<const float>(y), P<const int>(arg), P<const float>(den), T, F, Fp, eps,
                     P<float>(dm), P<float>(dc));
  hip_check(hipGetLastError(), "seq_norm_max_bwd launch");
}

void seq_conv_wgrad_pe(int dev, hipStream_t s, uintptr_t dm, uintptr_t arg, uintptr_t win, int64_t n, int T, int F,
                       int H, int k, int Kp, uintptr_t g, int64_t ldg, int64_t offW, int64_t offB) {
  need_dev(dev, "seq_conv_wgrad_pe");
  if (n <= 0 || n > 65535 || T <= 0 || F <= 0 || H <= 0 || k <= 0 || int64_t(k) * H > Kp)
    throw std::invalid_argument("seq_conv_wgrad_pe: bad shape");
  if (offW < 0 || offW + int64_t(F) * H * k > ldg || offB + F > ldg)
    throw std::invalid_argument("seq_conv_wgrad_pe: offsets outside a row of g");
  if (!dm || !arg || !win || !g) throw std::invalid_argument("seq_conv_wgrad_pe: null pointer");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  hipLaunchKernelGGL(seq_conv_wgrad_pe_kernel, dim3(unsigned((F + kWgF - 1) / kWgF), unsigned(n)), dim3(kThreads), 0,
                     s, P<const float>(dm), P<const int>(arg), P<const float>(win), n, T, F, H, k, Kp, P<float>(g),
                     ldg, offW, offB);
  hip_check(hipGetLastError(), "seq_conv_wgrad_pe launch");
}

void seq_hidden_bwd(int dev, hipStream_t s, uintptr_t dwin, int64_t ldw, uintptr_t win, int Kp, int64_t S, int T, int H,
                    int k, uintptr_t Wh, int D, uintptr_t da, uintptr_t de) {
  need_dev(dev, "seq_hidden_bwd");
  if (S <= 0 || T <= 0 || H <= 0 || k <= 0 || D <= 0 || int64_t(k) * H > Kp || int64_t(k) * H > ldw)
    throw std::invalid_argument("seq_hidden_bwd: bad shape");
  const size_t lds = size_t(kTok) * H * sizeof(float);
  if (lds > 48 * 1024) throw std::invalid_argument("seq_hidden_bwd: hidden dim too large");
  const int64_t ntok = S * T, nblk = (ntok + kTok - 1) / kTok;
  if (nblk > INT32_MAX) throw std::invalid_argument("seq_hidden_bwd: too many tokens");
  if (!dwin || !win || !Wh || !da || !de) throw std::invalid_argument("seq_hidden_bwd: null pointer");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  hipLaunchKernelGGL(seq_hidden_bwd_kernel, dim3(unsigned(nblk)), dim3(kThreads), lds, s, P<const float>(dwin), ldw,
                     P<const float>(win), Kp, ntok, T, H, k, P<const float>(Wh), D, P<float>(da), P<float>(de));
  hip_check(hipGetLastError(), "seq_hidden_bwd launch");
}

void seq_hidden_embed_grad_pe(int dev, hipStream_t s, uintptr_t da, uintptr_t de, uintptr_t tok, uintptr_t E,
                              int64_t V, int64_t n, int T, int H, int D, int64_t pad_idx, uintptr_t g, int64_t ldg,
                              int64_t offE, int64_t offWh, int64_t offBh) {
  need_dev(dev, "seq_hidden_embed_grad_pe");
  if (n <= 0 || n > 65535 || T <= 0 || H <= 0 || D <= 0 || V <= 0)
    throw std::invalid_argument("seq_hidden_embed_grad_pe: bad shape");
  if (offE < 0 || offE + V * D > ldg || offWh < 0 || offWh + int64_t(H) * D > ldg || offBh + H > ldg)
    throw std::invalid_argument("seq_hidden_embed_grad_pe: offsets outside a row of g");
  const size_t lds = size_t(3) * T * sizeof(int64_t);
  if (lds > 48 * 1024) throw std::invalid_argument("seq_hidden_embed_grad_pe: sentences too long");
  if (!da || !de || !tok || !E || !g) throw std::invalid_argument("seq_hidden_embed_grad_pe: null pointer");
  hip_check(hipSetDevice(dev), "hipSetDevice");
  const int64_t hd = int64_t(H) * D;
  if (hd > INT32_MAX) throw std::invalid_argument("seq_hidden_embed_grad_pe: hidden weight too large");
  hipLaunchKernelGGL(seq_hidden_wgrad_pe_kernel, dim3(unsigned((hd + kThreads - 1) / kThreads), unsigned(n)),
                     dim3(kThreads), 0, s, P<const float>(da), P<const int64_t>(tok), P<const float>(E), n, T, H, D,
                     P<float>(g), ldg, offWh, offBh);
  hip_check(hipGetLastError(), "seq_hidden_wgrad_pe launch");
  const int per = kThreads / 64;
  hipLaunchKernelGGL(seq_embed_grad_pe_kernel, dim3(unsigned((3 * T + per - 1) / per), unsigned(n)), dim3(kThreads),
                     lds, s, P<const float>(de), P<const int64_t>(tok), n, T, D, V, pad_idx, P<float>(g), ldg, offE);
  hip_check(hipGetLastError(), "seq_embed_grad_pe launch");
}

}  // namespace mpit
