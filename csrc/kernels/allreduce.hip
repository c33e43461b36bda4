// K13: the reducer of the window all-reduce (core/window.cpp Window::allreduce).
//     dst[j][i] = src[0][i] (op) src[1][i] (op) ... (op) src[ns-1][i]      i < n, j < nd
// ONE launch loads element i from all ns peers' HBM (IPC-mapped, xGMI), folds it left to
// right in the order given and stores it into all nd peers. The order is the member order of
// the window, so every rank computes the same bits whatever the bucketing; bf16 / fp16 sums
// are accumulated in fp32 and rounded once.
//
// Design (cdna_hip_programming.md Guideline 13, Appendix "Element-wise"): a streaming,
// HBM/xGMI-bound kernel. 256-thread blocks; each lane moves 16 B per source per step, all
// NS x U loads issued before the first combine (U independent vectors per lane, NS x U = 8
// vectors = 32 VGPRs of loads in flight), then 16-B stores to every destination. The pointer
// table travels by value in the kernel arguments (as gather.hip does): no device-side table.
// NS is a template parameter in {1, 2, 4, 8}: a source count in between re-loads the last
// source (an L2 hit) and skips it in the fold, so no load hides behind a runtime condition.
// The op is wave-uniform and switched once per vector, outside the fold.
// A scalar head and tail cover pointers that are not 16-B aligned (all of them must share
// their offset within 16 B for the vector body; otherwise the whole range runs scalar) and
// n that is no multiple of the vector width.
// Pair types (MAXLOC / MINLOC, peer_ops.h): the element is a whole pair and its pointers are
// aligned to the pair's largest member only (a float32 pair may sit at 4 mod 8), so a pair
// boundary need not be a 16-B address and the pointers need not share their offset. Their body
// is cut at dst[0] when a pair boundary of it is 16-B aligned and at element 0 otherwise, and
// every access of it is a 16-byte one where it falls (gfx950 executes a global dwordx4 access at
// any byte address; a second cache line per access at most). No pair is ever split between two
// lanes or between head, body and tail; the scalar parts move whole pairs.
// In place: every lane reads all the elements it owns before it writes any of them, and no
// two lanes own the same element, so dst[j] may be src[j].
// There is NO cross-rank communication in here: no flags, no spinning on peer memory.
// Ranks routinely share one GPU, where a spinning kernel can starve the peer it waits for.
#include <type_traits>

#include "ew.h"
#include "kernels.h"
#include "peer_ops.h"  // the element tags, widen / narrow / comb (shared with type_acc.hip), PeerTable, fold

// plain IEEE operations in the stated order: no contraction anywhere in this file
#pragma clang fp contract(off)

namespace mpit {
namespace {

constexpr int kPB = 256;
constexpr int kPGrid = 2048;

// elements [0, head) and [head + nvec*VE, n) run scalar (head == n, nvec == 0: all of them)
template <class Tag, int NS>
__global__ __launch_bounds__(kPB) void peer_reduce_kernel(PeerTable tab, int op, int64_t n, int64_t head,
                                                          int64_t nvec) {
  using S = typename Tag::S;
  using A = typename Tag::A;
  constexpr int VE = 16 / int(sizeof(S));
  constexpr int U = NS >= 8 ? 1 : (NS >= 4 ? 2 : 4);
  const int ns = tab.ns, nd = tab.nd;
  const int64_t tile = int64_t(kPB) * U;
  const int64_t ntiles = (nvec + tile - 1) / tile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint4 raw[U][NS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kPB + threadIdx.x;
      if (v < nvec) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const S* p = reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1]) + head;
          if constexpr (Tag::kPair) __builtin_memcpy(&raw[u][k], reinterpret_cast<const uint8_t*>(p) + v * 16, 16);
          else raw[u][k] = reinterpret_cast<const uint4*>(p)[v];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kPB + threadIdx.x;
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
        for (int j = 0; j < VE; ++j) o[j] = narrow<Tag>(x[0][j]);
        uint4 out;
        __builtin_memcpy(&out, o, 16);
        for (int j = 0; j < nd; ++j) {
          S* q = reinterpret_cast<S*>(tab.dst[j]) + head;
          if constexpr (Tag::kPair) __builtin_memcpy(reinterpret_cast<uint8_t*>(q) + v * 16, &out, 16);
          else reinterpret_cast<uint4*>(q)[v] = out;
        }
      }
    }
  }
  // scalar head and tail, spread over the grid
  const int64_t tail0 = head + nvec * VE;
  const int64_t nsc = head + (n - tail0);
  for (int64_t q = int64_t(blockIdx.x) * kPB + threadIdx.x; q < nsc; q += int64_t(gridDim.x) * kPB) {
    const int64_t i = q < head ? q : tail0 + (q - head);
    A x[NS][1];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k][0] = widen<Tag>(reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1])[i]);
    fold_op<Tag, NS, 1>(op, x, ns);
    const S o = narrow<Tag>(x[0][0]);
    for (int j = 0; j < nd; ++j) reinterpret_cast<S*>(tab.dst[j])[i] = o;
  }
}

template <class Tag>
void host_reduce(int op, const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts, int64_t n) {
  using S = typename Tag::S;
  using A = typename Tag::A;
  const int ns = int(srcs.size());
  for (int64_t i = 0; i < n; ++i) {
    A x[kPeerMax][1];
    for (int k = 0; k < ns; ++k) x[k][0] = widen<Tag>(reinterpret_cast<const S*>(srcs[size_t(k)])[i]);
    fold_op<Tag, kPeerMax, 1>(op, x, ns);
    const S o = narrow<Tag>(x[0][0]);
    for (uintptr_t d : dsts) reinterpret_cast<S*>(d)[i] = o;
  }
}

template <class Tag>
void launch(int dev, hipStream_t s, int op, const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts,
            int64_t n) {
  using S = typename Tag::S;
  if (dev < 0) {
    host_reduce<Tag>(op, srcs, dsts, n);
    return;
  }
  constexpr int VE = 16 / int(sizeof(S));
  PeerTable tab{};
  tab.ns = int32_t(srcs.size());
  tab.nd = int32_t(dsts.size());
  const uintptr_t mis = srcs[0] & 15;
  bool vec = mis % sizeof(S) == 0;
  for (size_t k = 0; k < srcs.size(); ++k) {
    tab.src[k] = srcs[k];
    vec = vec && (srcs[k] & 15) == mis;
  }
  for (size_t k = 0; k < dsts.size(); ++k) {
    tab.dst[k] = dsts[k];
    vec = vec && (dsts[k] & 15) == mis;
  }
  int64_t head = n, nvec = 0;
  if constexpr (Tag::kPair) {  // accessed where it falls: nothing to share, and never a split pair
    const uintptr_t dm = dsts[0] & 15;
    head = dm % sizeof(S) == 0 ? std::min<int64_t>(n, int64_t((16 - dm) & 15) / int64_t(sizeof(S))) : 0;
    nvec = (n - head) / VE;
  } else if (vec) {
    head = std::min<int64_t>(n, int64_t((16 - mis) & 15) / int64_t(sizeof(S)));
    nvec = (n - head) / VE;
  }
  const int ns = tab.ns;
  const int NS = ns <= 1 ? 1 : (ns <= 2 ? 2 : (ns <= 4 ? 4 : 8));
  const int U = NS >= 8 ? 1 : (NS >= 4 ? 2 : 4);
  const int64_t tile = int64_t(kPB) * U;
  const int64_t nsc = n - nvec * VE;
  const int64_t want = std::max((nvec + tile - 1) / tile, (nsc + kPB - 1) / kPB);
  const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(want, kPGrid)));
  hip_check(hipSetDevice(dev), "hipSetDevice");
  switch (NS) {
    case 1: hipLaunchKernelGGL((peer_reduce_kernel<Tag, 1>), dim3(grid), dim3(kPB), 0, s, tab, op, n, head, nvec); break;
    case 2: hipLaunchKernelGGL((peer_reduce_kernel<Tag, 2>), dim3(grid), dim3(kPB), 0, s, tab, op, n, head, nvec); break;
    case 4: hipLaunchKernelGGL((peer_reduce_kernel<Tag, 4>), dim3(grid), dim3(kPB), 0, s, tab, op, n, head, nvec); break;
    default: hipLaunchKernelGGL((peer_reduce_kernel<Tag, 8>), dim3(grid), dim3(kPB), 0, s, tab, op, n, head, nvec); break;
  }
  hip_check(hipGetLastError(), "peer_reduce launch");
}

}  // namespace

bool peer_reduce_supported(int op, int dtype) {
  if (peer_dtype_is_pair(dtype)) return op == kPrMaxloc || op == kPrMinloc;
  if (op < 0 || op >= kPrOps || dtype < 0 || dtype >= kPrDtypes) return false;
  const bool integer = dtype == kPrI32 || dtype == kPrI64 || dtype == kPrU8;
  return op < kPrBand || integer;
}

bool peer_dtype_is_pair(int dtype) {
  return (dtype >= kPrPair && dtype < kPrPair + kPrDtypes) || (dtype >= kPrFloatInt && dtype <= kPrLongInt);
}

int peer_dtype_align(int dtype) {
  switch (dtype) {
    case kPrF32: case kPrI32: case kPrFloatInt: return 4;
    case kPrBf16: case kPrF16: return 2;
    case kPrF64: case kPrI64: case kPrDoubleInt: case kPrLongInt: return 8;
    case kPrU8: return 1;
    default:
      if (dtype >= kPrPair && dtype < kPrPair + kPrDtypes) return peer_dtype_align(dtype - kPrPair);
      throw std::invalid_argument("peer_reduce: unknown dtype");
  }
}

int peer_dtype_size(int dtype) {
  if (dtype >= kPrPair && dtype < kPrPair + kPrDtypes) return 2 * peer_dtype_align(dtype - kPrPair);
  if (dtype == kPrFloatInt) return 8;
  if (dtype == kPrDoubleInt || dtype == kPrLongInt) return 16;
  return peer_dtype_align(dtype);
}

void peer_reduce(int dev, hipStream_t s, int op, int dtype, const std::vector<uintptr_t>& srcs,
                 const std::vector<uintptr_t>& dsts, int64_t n) {
  if (!peer_reduce_supported(op, dtype)) throw std::invalid_argument("peer_reduce: unsupported (op, dtype)");
  if (srcs.empty() || srcs.size() > size_t(kPeerMax) || dsts.empty() || dsts.size() > size_t(kPeerMax))
    throw std::invalid_argument("peer_reduce: 1..8 sources and destinations");
  const uintptr_t es = uintptr_t(peer_dtype_align(dtype));
  for (uintptr_t p : srcs)
    if (!p || p % es) throw std::invalid_argument("peer_reduce: null or misaligned source");
  for (uintptr_t p : dsts)
    if (!p || p % es) throw std::invalid_argument("peer_reduce: null or misaligned destination");
  if (n <= 0) return;
  with_peer_tag(dtype, [&](auto tag) { launch<decltype(tag)>(dev, s, op, srcs, dsts, n); });
}

}  // namespace mpit
