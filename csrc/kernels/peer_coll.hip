// The kernels of the window collectives (core/window.cpp Window::pull_gather, pull_fold,
// scan), one launch each between the two barriers of the protocol.
//   peer_gather   dst[g][b] = src[g][b]                      b < bytes[g], up to 8 segments
//   peer_fold     dst[i]    = src[0][i] op ... op src[ns-1][i]          one local destination
//   peer_scan     dst[j][i] = src[0][i] op ... op src[j][i]             every j < ns (inclusive)
//                 dst[j][i] = src[0][i] op ... op src[j-1][i]           j >= 1 (exclusive)
// The sources are usually other members' IPC mappings, at whatever base sym_register exposed
// them: nothing in here assumes that the pointers of a call share their offset within 16 B.
//
// Design (the rules of allreduce.hip): streaming, HBM/xGMI-bound kernels; 256-thread blocks;
// each lane moves 16 B per pointer per step and all loads of a step are issued before the first
// combine or store; the pointer table travels by value in the kernel arguments. The vector
// body is cut so that the destination (peer_gather, peer_fold: one per segment / call;
// peer_scan: the first one written) is 16-B aligned; every other pointer is accessed where it
// falls, through a 16-byte __builtin_memcpy (gfx950 executes a global dwordx4 access at any byte
// address; it costs a second cache line per access at most, never a scalar loop). Heads and
// tails run scalar. A pair type (MAXLOC / MINLOC) is aligned to its largest member only, so its
// destination may have no 16-B aligned pair boundary at all (a float32 pair at 4 mod 8): then the
// body starts at element 0 and the destination too is stored where it falls. No pair is split.
// peer_gather: blocks find their segment in a prefix table of per-segment tile counts, a
// wave-uniform scan of at most 8 entries, so a long segment and a 3-byte one share the grid.
// peer_scan: the accumulator stays wide across the chain (a 16-bit float prefix j is the fp32
// fold of 0..j rounded once); a lane reads every source element it owns before it stores any,
// and no two lanes own the same element, so dst[j] may be src[j].
// There is NO cross-rank communication in here: no flags, no spinning on peer memory.
#include <cstring>
#include <type_traits>

#include "ew.h"
#include "kernels.h"
#include "peer_ops.h"  // the element tags, widen / narrow / comb, PeerTable, fold: the all-reduce's bits

// plain IEEE operations in the stated order: no contraction anywhere in this file
#pragma clang fp contract(off)

namespace mpit {
namespace {

constexpr int kCB = 256;
constexpr int kCGrid = 2048;  // the production cap of the grid (max_blocks == 0)
constexpr int kGU = 4;        // peer_gather: vectors per lane per tile (16 KiB per tile)

unsigned grid_for(int64_t want, int max_blocks) {
  const int64_t cap = max_blocks > 0 ? max_blocks : kCGrid;
  return unsigned(std::max<int64_t>(1, std::min<int64_t>(want, cap)));
}

MPIT_HD uint4 load16(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
MPIT_HD void store16(uint8_t* p, const uint4& v) { __builtin_memcpy(p, &v, 16); }

// narrow() of an fp16 accumulator, kept apart from the multiply that made it. Left to itself the
// gfx950 back end turns narrow(widen(a) * b) into one v_fma_mixlo_f16 a, b, +0, and (-0) + (+0) is
// +0: a PROD whose exact result is -0 would lose its sign (seen in the scalar path of peer_scan).
// The empty statement emits nothing; it only makes the value opaque at this point.
template <class Tag>
MPIT_HD typename Tag::S narrow_acc(typename Tag::A v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (std::is_same_v<Tag, TF16>) asm volatile("" : "+v"(v));
#endif
  return narrow<Tag>(v);
}

// ------------------------------------------------------------------ peer_gather
struct GatherTable {
  uint64_t src[kPeerMax];
  uint64_t dst[kPeerMax];
  int64_t bytes[kPeerMax];
  int64_t tiles[kPeerMax];  // inclusive prefix of the per-segment tile counts
  int32_t ng;
};

MPIT_HD int64_t gather_head(uint64_t dst, int64_t bytes) {
  const int64_t h = int64_t((16 - (dst & 15)) & 15);
  return h < bytes ? h : bytes;
}

// tiles of a segment: one per kCB * kGU vectors of its body, at least one when it has bytes
// (tile 0 also moves the head and the tail, fewer than 16 bytes each)
int64_t gather_tiles(uint64_t dst, int64_t bytes) {
  if (bytes <= 0) return 0;
  const int64_t nvec = (bytes - gather_head(dst, bytes)) / 16;
  return std::max<int64_t>(1, (nvec + kCB * kGU - 1) / (kCB * kGU));
}

__global__ __launch_bounds__(kCB) void peer_gather_kernel(GatherTable tab) {
  const int ng = tab.ng;
  const int64_t total = tab.tiles[ng - 1];
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    int g = 0;
    while (g < ng - 1 && t >= tab.tiles[g]) ++g;  // wave-uniform, at most 7 steps
    const int64_t lt = t - (g ? tab.tiles[g - 1] : 0);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(tab.src[g]);
    uint8_t* dst = reinterpret_cast<uint8_t*>(tab.dst[g]);
    const int64_t bytes = tab.bytes[g];
    const int64_t head = gather_head(tab.dst[g], bytes);
    const int64_t nvec = (bytes - head) / 16;
    uint4 raw[kGU];
#pragma unroll
    for (int u = 0; u < kGU; ++u) {
      const int64_t v = (lt * kGU + u) * kCB + threadIdx.x;
      if (v < nvec) raw[u] = load16(src + head + v * 16);  // where it falls
    }
#pragma unroll
    for (int u = 0; u < kGU; ++u) {
      const int64_t v = (lt * kGU + u) * kCB + threadIdx.x;
      if (v < nvec) *reinterpret_cast<uint4*>(dst + head + v * 16) = raw[u];  // 16-B aligned
    }
    if (lt == 0) {  // head: lanes 0..14, tail: lanes 64..78 (another wave)
      const int64_t tail0 = head + nvec * 16;
      const int64_t q = threadIdx.x;
      if (q < head) dst[q] = src[q];
      else if (q >= 64 && tail0 + (q - 64) < bytes) dst[tail0 + (q - 64)] = src[tail0 + (q - 64)];
    }
  }
}

// ------------------------------------------------------------------ peer_fold
// elements [0, head) and [head + nvec*VE, n) run scalar; the body's vector v is elements
// [head + v*VE, head + (v+1)*VE): 16-B aligned in dst, wherever they fall in every source
template <class Tag, int NS>
__global__ __launch_bounds__(kCB) void peer_fold_kernel(PeerTable tab, int op, int64_t n, int64_t head, int64_t nvec) {
  using S = typename Tag::S;
  using A = typename Tag::A;
  constexpr int VE = 16 / int(sizeof(S));
  constexpr int U = NS >= 8 ? 1 : (NS >= 4 ? 2 : 4);
  const int ns = tab.ns;
  S* dst = reinterpret_cast<S*>(tab.dst[0]);
  const int64_t tile = int64_t(kCB) * U;
  const int64_t ntiles = (nvec + tile - 1) / tile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint4 raw[U][NS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kCB + threadIdx.x;
      if (v < nvec) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const S* p = reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1]) + head + v * VE;
          raw[u][k] = load16(reinterpret_cast<const uint8_t*>(p));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kCB + threadIdx.x;
      if (v < nvec) {
        A x[NS][VE];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          S e[VE];
          __builtin_memcpy(e, &raw[u][k], 16);
#pragma unroll
          for (int j = 0; j < VE; ++j) x[k][j] = widen<Tag>(e[j]);
        }
        fold_op<Tag, NS, VE>(op, x, ns);
        S o[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) o[j] = narrow_acc<Tag>(x[0][j]);
        uint4 out;
        __builtin_memcpy(&out, o, 16);
        if constexpr (Tag::kPair) store16(reinterpret_cast<uint8_t*>(dst + head + v * VE), out);  // where it falls
        else *reinterpret_cast<uint4*>(dst + head + v * VE) = out;
      }
    }
  }
  const int64_t tail0 = head + nvec * VE;
  const int64_t nsc = head + (n - tail0);
  for (int64_t q = int64_t(blockIdx.x) * kCB + threadIdx.x; q < nsc; q += int64_t(gridDim.x) * kCB) {
    const int64_t i = q < head ? q : tail0 + (q - head);
    A x[NS][1];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k][0] = widen<Tag>(reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1])[i]);
    fold_op<Tag, NS, 1>(op, x, ns);
    dst[i] = narrow_acc<Tag>(x[0][0]);
  }
}

// ------------------------------------------------------------------ peer_scan
// The chain over one lane's VE elements of all sources, already loaded: stores prefix k into
// put(k, ...) for k < ns (inclusive) or 1 <= k < ns (exclusive, the fold of 0..k-1).
template <class Tag, int OP, int NS, int VE, class Put>
MPIT_HD void scan_chain(const typename Tag::S (&e)[NS][VE], int ns, bool excl, Put&& put) {
  using S = typename Tag::S;
  using A = typename Tag::A;
  A acc[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) acc[j] = widen<Tag>(e[0][j]);
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    if (k < ns) {
      if (k > 0 && !excl) {
#pragma unroll
        for (int j = 0; j < VE; ++j) acc[j] = comb<Tag, OP>(acc[j], widen<Tag>(e[k][j]));
      }
      if (k > 0 || !excl) {
        S o[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) o[j] = narrow_acc<Tag>(acc[j]);
        put(k, o);
      }
      if (k > 0 && excl) {
#pragma unroll
        for (int j = 0; j < VE; ++j) acc[j] = comb<Tag, OP>(acc[j], widen<Tag>(e[k][j]));
      }
    }
  }
}

template <class Tag, int NS, int VE, class Put>
MPIT_HD void scan_op(int op, const typename Tag::S (&e)[NS][VE], int ns, bool excl, Put&& put) {
  if constexpr (Tag::kPair) {
    if (op == kPrMaxloc) scan_chain<Tag, kPrMaxloc, NS, VE>(e, ns, excl, put);
    else scan_chain<Tag, kPrMinloc, NS, VE>(e, ns, excl, put);
    return;
  }
  switch (op) {
    case kPrSum: scan_chain<Tag, kPrSum, NS, VE>(e, ns, excl, put); break;
    case kPrProd: scan_chain<Tag, kPrProd, NS, VE>(e, ns, excl, put); break;
    case kPrMax: scan_chain<Tag, kPrMax, NS, VE>(e, ns, excl, put); break;
    case kPrMin: scan_chain<Tag, kPrMin, NS, VE>(e, ns, excl, put); break;
    case kPrLand: scan_chain<Tag, kPrLand, NS, VE>(e, ns, excl, put); break;
    case kPrLor: scan_chain<Tag, kPrLor, NS, VE>(e, ns, excl, put); break;
    case kPrLxor: scan_chain<Tag, kPrLxor, NS, VE>(e, ns, excl, put); break;
    default:
      if constexpr (Tag::kInt && !Tag::kPair) {
        if (op == kPrBand) scan_chain<Tag, kPrBand, NS, VE>(e, ns, excl, put);
        else if (op == kPrBor) scan_chain<Tag, kPrBor, NS, VE>(e, ns, excl, put);
        else scan_chain<Tag, kPrBxor, NS, VE>(e, ns, excl, put);
      }
      break;
  }
}

// the body's vector v is 16-B aligned in the first destination written; every other pointer is accessed where it falls
template <class Tag, int NS>
__global__ __launch_bounds__(kCB) void peer_scan_kernel(PeerTable tab, int op, int excl, int64_t n, int64_t head,
                                                        int64_t nvec) {
  using S = typename Tag::S;
  constexpr int VE = 16 / int(sizeof(S));
  constexpr int U = NS >= 8 ? 1 : 2;
  const int ns = tab.ns;
  const int64_t tile = int64_t(kCB) * U;
  const int64_t ntiles = (nvec + tile - 1) / tile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint4 raw[U][NS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kCB + threadIdx.x;
      if (v < nvec) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const S* p = reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1]) + head + v * VE;
          raw[u][k] = load16(reinterpret_cast<const uint8_t*>(p));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kCB + threadIdx.x;
      if (v < nvec) {
        S e[NS][VE];
#pragma unroll
        for (int k = 0; k < NS; ++k) __builtin_memcpy(e[k], &raw[u][k], 16);
        const int64_t at = head + v * VE;
        scan_op<Tag, NS, VE>(op, e, ns, excl != 0, [&](int k, const S(&o)[VE]) {
          uint4 out;
          __builtin_memcpy(&out, o, 16);
          store16(reinterpret_cast<uint8_t*>(reinterpret_cast<S*>(tab.dst[k]) + at), out);
        });
      }
    }
  }
  const int64_t tail0 = head + nvec * VE;
  const int64_t nsc = head + (n - tail0);
  for (int64_t q = int64_t(blockIdx.x) * kCB + threadIdx.x; q < nsc; q += int64_t(gridDim.x) * kCB) {
    const int64_t i = q < head ? q : tail0 + (q - head);
    S e[NS][1];
#pragma unroll
    for (int k = 0; k < NS; ++k) e[k][0] = reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1])[i];
    scan_op<Tag, NS, 1>(op, e, ns, excl != 0, [&](int k, const S(&o)[1]) { reinterpret_cast<S*>(tab.dst[k])[i] = o[0]; });
  }
}

// ------------------------------------------------------------------ host twins and launchers
template <class Tag>
void host_fold(int op, const std::vector<uintptr_t>& srcs, uintptr_t dst, int64_t n) {
  using S = typename Tag::S;
  using A = typename Tag::A;
  const int ns = int(srcs.size());
  for (int64_t i = 0; i < n; ++i) {
    A x[kPeerMax][1];
    for (int k = 0; k < ns; ++k) x[k][0] = widen<Tag>(reinterpret_cast<const S*>(srcs[size_t(k)])[i]);
    fold_op<Tag, kPeerMax, 1>(op, x, ns);
    reinterpret_cast<S*>(dst)[i] = narrow<Tag>(x[0][0]);
  }
}

template <class Tag>
void host_scan(int op, bool excl, const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts, int64_t n) {
  using S = typename Tag::S;
  const int ns = int(srcs.size());
  for (int64_t i = 0; i < n; ++i) {
    S e[kPeerMax][1];
    for (int k = 0; k < kPeerMax; ++k) e[k][0] = reinterpret_cast<const S*>(srcs[size_t(k < ns ? k : ns - 1)])[i];
    scan_op<Tag, kPeerMax, 1>(op, e, ns, excl,
                              [&](int k, const S(&o)[1]) { reinterpret_cast<S*>(dsts[size_t(k)])[i] = o[0]; });
  }
}

// the cut of n elements at a destination: scalar head up to its next 16-B address, vectors, tail
// (a pair type whose element boundaries never meet a 16-B address: no head)
template <class S>
void cut(uintptr_t dst, int64_t n, int64_t* head, int64_t* nvec) {
  constexpr int VE = 16 / int(sizeof(S));
  *head = (dst & 15) % sizeof(S) ? 0 : std::min<int64_t>(n, int64_t((16 - (dst & 15)) & 15) / int64_t(sizeof(S)));
  *nvec = (n - *head) / VE;
}

template <class Tag>
void launch_fold(int dev, hipStream_t s, int op, const std::vector<uintptr_t>& srcs, uintptr_t dst, int64_t n,
                 int max_blocks) {
  using S = typename Tag::S;
  if (dev < 0) {
    host_fold<Tag>(op, srcs, dst, n);
    return;
  }
  constexpr int VE = 16 / int(sizeof(S));
  PeerTable tab{};
  tab.ns = int32_t(srcs.size());
  tab.nd = 1;
  for (size_t k = 0; k < srcs.size(); ++k) tab.src[k] = srcs[k];
  tab.dst[0] = dst;
  int64_t head, nvec;
  cut<S>(dst, n, &head, &nvec);
  const int ns = tab.ns;
  const int NS = ns <= 1 ? 1 : (ns <= 2 ? 2 : (ns <= 4 ? 4 : 8));
  const int U = NS >= 8 ? 1 : (NS >= 4 ? 2 : 4);
  const int64_t tile = int64_t(kCB) * U;
  const int64_t nsc = n - nvec * VE;
  const unsigned grid = grid_for(std::max((nvec + tile - 1) / tile, (nsc + kCB - 1) / kCB), max_blocks);
  hip_check(hipSetDevice(dev), "hipSetDevice");
  switch (NS) {
    case 1: hipLaunchKernelGGL((peer_fold_kernel<Tag, 1>), dim3(grid), dim3(kCB), 0, s, tab, op, n, head, nvec); break;
    case 2: hipLaunchKernelGGL((peer_fold_kernel<Tag, 2>), dim3(grid), dim3(kCB), 0, s, tab, op, n, head, nvec); break;
    case 4: hipLaunchKernelGGL((peer_fold_kernel<Tag, 4>), dim3(grid), dim3(kCB), 0, s, tab, op, n, head, nvec); break;
    default: hipLaunchKernelGGL((peer_fold_kernel<Tag, 8>), dim3(grid), dim3(kCB), 0, s, tab, op, n, head, nvec); break;
  }
  hip_check(hipGetLastError(), "peer_fold launch");
}

template <class Tag>
void launch_scan(int dev, hipStream_t s, int op, bool excl, const std::vector<uintptr_t>& srcs,
                 const std::vector<uintptr_t>& dsts, int64_t n, int max_blocks) {
  using S = typename Tag::S;
  if (dev < 0) {
    host_scan<Tag>(op, excl, srcs, dsts, n);
    return;
  }
  constexpr int VE = 16 / int(sizeof(S));
  PeerTable tab{};
  tab.ns = tab.nd = int32_t(srcs.size());
  for (size_t k = 0; k < srcs.size(); ++k) {
    tab.src[k] = srcs[k];
    tab.dst[k] = dsts[k];
  }
  const int ns = tab.ns;
  if (excl && ns == 1) return;  // dst[0] is never written
  int64_t head, nvec;
  cut<S>(dsts[excl ? 1 : 0], n, &head, &nvec);  // the first destination written
  const int NS = ns <= 1 ? 1 : (ns <= 2 ? 2 : (ns <= 4 ? 4 : 8));
  const int U = NS >= 8 ? 1 : 2;
  const int64_t tile = int64_t(kCB) * U;
  const int64_t nsc = n - nvec * VE;
  const unsigned grid = grid_for(std::max((nvec + tile - 1) / tile, (nsc + kCB - 1) / kCB), max_blocks);
  const int ex = excl ? 1 : 0;
  hip_check(hipSetDevice(dev), "hipSetDevice");
  switch (NS) {
    case 1: hipLaunchKernelGGL((peer_scan_kernel<Tag, 1>), dim3(grid), dim3(kCB), 0, s, tab, op, ex, n, head, nvec); break;
    case 2: hipLaunchKernelGGL((peer_scan_kernel<Tag, 2>), dim3(grid), dim3(kCB), 0, s, tab, op, ex, n, head, nvec); break;
    case 4: hipLaunchKernelGGL((peer_scan_kernel<Tag, 4>), dim3(grid), dim3(kCB), 0, s, tab, op, ex, n, head, nvec); break;
    default: hipLaunchKernelGGL((peer_scan_kernel<Tag, 8>), dim3(grid), dim3(kCB), 0, s, tab, op, ex, n, head, nvec); break;
  }
  hip_check(hipGetLastError(), "peer_scan launch");
}

void check_fold_args(const char* who, int op, int dtype, const std::vector<uintptr_t>& srcs,
                     const std::vector<uintptr_t>& dsts) {
  const std::string w(who);
  if (!peer_reduce_supported(op, dtype)) throw std::invalid_argument(w + ": unsupported (op, dtype)");
  if (srcs.empty() || srcs.size() > size_t(kPeerMax)) throw std::invalid_argument(w + ": 1..8 sources");
  const uintptr_t es = uintptr_t(peer_dtype_align(dtype));
  for (uintptr_t p : srcs)
    if (!p || p % es) throw std::invalid_argument(w + ": null or misaligned source");
  for (uintptr_t p : dsts)
    if (!p || p % es) throw std::invalid_argument(w + ": null or misaligned destination");
}

}  // namespace

void peer_gather(int dev, hipStream_t s, const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts,
                 const std::vector<int64_t>& bytes, int max_blocks) {
  if (srcs.size() != dsts.size() || srcs.size() != bytes.size() || srcs.size() > size_t(kPeerMax))
    throw std::invalid_argument("peer_gather: up to 8 segments of (source, destination, bytes)");
  GatherTable tab{};
  int ng = 0;
  int64_t total = 0;
  for (size_t g = 0; g < srcs.size(); ++g) {
    if (bytes[g] < 0) throw std::invalid_argument("peer_gather: negative length");
    if (bytes[g] == 0 || srcs[g] == dsts[g]) continue;  // nothing to move
    if (!srcs[g] || !dsts[g]) throw std::invalid_argument("peer_gather: null source or destination");
    if (dev < 0) {
      std::memcpy(reinterpret_cast<void*>(dsts[g]), reinterpret_cast<const void*>(srcs[g]), size_t(bytes[g]));
      continue;
    }
    total += gather_tiles(dsts[g], bytes[g]);
    tab.src[ng] = srcs[g];
    tab.dst[ng] = dsts[g];
    tab.bytes[ng] = bytes[g];
    tab.tiles[ng] = total;
    ++ng;
  }
  if (dev < 0 || ng == 0) return;
  tab.ng = ng;
  hip_check(hipSetDevice(dev), "hipSetDevice");
  hipLaunchKernelGGL(peer_gather_kernel, dim3(grid_for(total, max_blocks)), dim3(kCB), 0, s, tab);
  hip_check(hipGetLastError(), "peer_gather launch");
}

void peer_fold(int dev, hipStream_t s, int op, int dtype, const std::vector<uintptr_t>& srcs, uintptr_t dst, int64_t n,
               int max_blocks) {
  check_fold_args("peer_fold", op, dtype, srcs, {dst});
  if (n <= 0) return;
  with_peer_tag(dtype, [&](auto tag) { launch_fold<decltype(tag)>(dev, s, op, srcs, dst, n, max_blocks); });
}

void peer_scan(int dev, hipStream_t s, int op, int dtype, bool exclusive, const std::vector<uintptr_t>& srcs,
               const std::vector<uintptr_t>& dsts, int64_t n, int max_blocks) {
  if (dsts.size() != srcs.size()) throw std::invalid_argument("peer_scan: one destination per source");
  // (the exclusive form never writes dst[0]: it may be anything, 0 included)
  check_fold_args("peer_scan", op, dtype, srcs,
                  exclusive && !dsts.empty() ? std::vector<uintptr_t>(dsts.begin() + 1, dsts.end()) : dsts);
  if (n <= 0) return;
  with_peer_tag(dtype,
                [&](auto tag) { launch_scan<decltype(tag)>(dev, s, op, exclusive, srcs, dsts, n, max_blocks); });
}

}  // namespace mpit
