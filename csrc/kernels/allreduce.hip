// K13: the reducer of the window all-reduce (core/window.cpp Window::allreduce) and of the
// reducing window collectives (Window::pull_fold).
//   peer_reduce   dst[j][i] = src[0][i] (op) src[1][i] (op) ... (op) src[ns-1][i]      i < n, j < nd
//   peer_fold     peer_reduce with one destination, the body cut at it
// ONE launch loads element i from all ns peers' HBM (IPC-mapped, xGMI), folds it left to
// right in the order given and stores it into all nd peers. The order is the member order of
// the window, so every rank computes the same bits whatever the bucketing; bf16 / fp16 sums
// are accumulated in fp32 and rounded once (narrow_acc).
//
// One kernel template, peer_reduce_kernel<Tag, NS, ONE>, serves both entry points; it follows
// the rules of peer_stream.h (tile loop, all NS x U loads before the first combine, scalar head
// and tail) but spells the frame out, for its registers (see the kernel). load16 / store16,
// narrow_acc, cut, the argument check and the launcher are peer_stream.h's. The op is
// wave-uniform and switched once per vector, outside the fold (with_peer_op, peer_ops.h).
// NS x U = 8 vectors = 32 VGPRs of loads in flight.
// Cut rules. peer_reduce, scalar types: a vector body only when every pointer shares its offset
// within 16 B (then every access of the body is 16-B aligned), otherwise the whole range runs
// scalar. peer_reduce, pair types (MAXLOC / MINLOC, peer_ops.h): the element is a whole pair and
// its pointers are aligned to the pair's largest member only (a float32 pair may sit at 4 mod 8),
// so a pair boundary need not be a 16-B address and the pointers need not share their offset: the
// body is cut at dst[0] when a pair boundary of it is 16-B aligned and at element 0 otherwise.
// peer_fold: cut at its destination, every source accessed where it falls, so sources at other
// alignments (other members' IPC mappings) never cost a scalar loop. No pair is ever split
// between two lanes or between head, body and tail; the scalar parts move whole pairs.
// In place: every lane reads all the elements it owns before it writes any of them, and no
// two lanes own the same element, so dst[j] may be src[j].
// There is NO cross-rank communication in here: no flags, no spinning on peer memory.
// Ranks routinely share one GPU, where a spinning kernel can starve the peer it waits for.
#include <type_traits>

#include "ew.h"
#include "kernels.h"
#include "peer_ops.h"     // the element tags, widen / narrow / comb (shared with type_acc.hip), PeerTable, fold
#include "peer_stream.h"  // the streaming skeleton and its launcher (shared with peer_coll.hip)

// plain IEEE operations in the stated order: no contraction anywhere in this file
#pragma clang fp contract(off)

namespace mpit {
namespace {

constexpr int reduce_u(int NS) { return NS >= 8 ? 1 : (NS >= 4 ? 2 : 4); }

// out[0..VE) = e[0][.] op e[1][.] op ... op e[ns-1][.], accumulated wide and narrowed once
template <class Tag, int NS, int VE>
MPIT_HD void reduce_elems(int op, const typename Tag::S (&e)[NS][VE], int ns, typename Tag::S (&o)[VE]) {
  typename Tag::A x[NS][VE];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
#pragma unroll
    for (int j = 0; j < VE; ++j) x[k][j] = widen<Tag>(e[k][j]);
  }
  fold_op<Tag, NS, VE>(op, x, ns);
#pragma unroll
  for (int j = 0; j < VE; ++j) o[j] = narrow_acc<Tag>(x[0][j]);
}

// ONE: dst[0] is the only destination (peer_fold), which spares the nd loop its registers.
// This kernel spells peer_stream's frame out instead of running on it: with the body behind a
// lambda, and with the loaded elements staged in an array before they are widened, the register
// allocator gave ten instances up to 40 VGPRs more than the parent's kernels had
// (profiles/peer_stream_refactor.md). Widening source by source straight from the loaded vectors,
// and 16-B aligned typed accesses where peer_reduce's scalar types guarantee them, keep them.
template <class Tag, int NS, bool ONE>
__global__ __launch_bounds__(kPeerBlock) void peer_reduce_kernel(PeerTable tab, int op, int64_t n, int64_t head,
                                                                 int64_t nvec) {
  using S = typename Tag::S;
  using A = typename Tag::A;
  constexpr int VE = 16 / int(sizeof(S));
  constexpr int U = reduce_u(NS);
  constexpr bool kTyped = !ONE && !Tag::kPair;  // every pointer shares its offset: the body is 16-B aligned in all
  const int ns = tab.ns, nd = ONE ? 1 : tab.nd;
  const int64_t tile = int64_t(kPeerBlock) * U;
  const int64_t ntiles = (nvec + tile - 1) / tile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint4 raw[U][NS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kPeerBlock + threadIdx.x;
      if (v < nvec) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const S* p = reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1]) + head;
          if constexpr (kTyped) raw[u][k] = reinterpret_cast<const uint4*>(p)[v];
          else raw[u][k] = load16(reinterpret_cast<const uint8_t*>(p) + v * 16);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kPeerBlock + threadIdx.x;
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
        for (int j = 0; j < nd; ++j) {
          S* q = reinterpret_cast<S*>(tab.dst[j]) + head;
          if constexpr (kTyped) reinterpret_cast<uint4*>(q)[v] = out;
          else store16(reinterpret_cast<uint8_t*>(q) + v * 16, out);
        }
      }
    }
  }
  // scalar head and tail, spread over the grid
  const int64_t tail0 = head + nvec * VE;
  const int64_t nsc = head + (n - tail0);
  for (int64_t q = int64_t(blockIdx.x) * kPeerBlock + threadIdx.x; q < nsc; q += int64_t(gridDim.x) * kPeerBlock) {
    const int64_t i = q < head ? q : tail0 + (q - head);
    A x[NS][1];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k][0] = widen<Tag>(reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1])[i]);
    fold_op<Tag, NS, 1>(op, x, ns);
    const S o = narrow_acc<Tag>(x[0][0]);
    for (int j = 0; j < nd; ++j) reinterpret_cast<S*>(tab.dst[j])[i] = o;
  }
}

template <class Tag>
void host_reduce(int op, const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts, int64_t n) {
  using S = typename Tag::S;
  const int ns = int(srcs.size());
  for (int64_t i = 0; i < n; ++i) {
    S e[kPeerMax][1] = {}, o[1];  // (entries past ns are widened but never folded)
    for (int k = 0; k < ns; ++k) e[k][0] = reinterpret_cast<const S*>(srcs[size_t(k)])[i];
    reduce_elems<Tag>(op, e, ns, o);
    for (uintptr_t d : dsts) reinterpret_cast<S*>(d)[i] = o[0];
  }
}

// one: peer_fold (cut at the destination); otherwise peer_reduce's rules
template <class Tag>
void launch(int dev, hipStream_t s, int op, const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts,
            int64_t n, bool one, int max_blocks) {
  using S = typename Tag::S;
  if (dev < 0) {
    host_reduce<Tag>(op, srcs, dsts, n);
    return;
  }
  const PeerTable tab = peer_table(srcs, dsts);
  int64_t head = n, nvec = 0;
  if (one || Tag::kPair) {  // sources accessed where they fall: nothing to share
    cut<S>(dsts[0], n, &head, &nvec);
  } else {
    bool vec = true;
    for (uintptr_t p : srcs) vec = vec && (p & 15) == (dsts[0] & 15);
    for (uintptr_t p : dsts) vec = vec && (p & 15) == (dsts[0] & 15);
    if (vec) cut<S>(dsts[0], n, &head, &nvec);
  }
  peer_launch<S>(dev, one ? "peer_fold launch" : "peer_reduce launch", tab.ns, n, nvec, max_blocks, reduce_u,
                 [&](auto NS, dim3 grid) {
                   auto k = one ? peer_reduce_kernel<Tag, decltype(NS)::value, true>
                                : peer_reduce_kernel<Tag, decltype(NS)::value, false>;
                   hipLaunchKernelGGL(k, grid, dim3(kPeerBlock), 0, s, tab, op, n, head, nvec);
                 });
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
  check_fold_args("peer_reduce", op, dtype, srcs, dsts, true);
  if (n <= 0) return;
  with_peer_tag(dtype, [&](auto tag) { launch<decltype(tag)>(dev, s, op, srcs, dsts, n, false, 0); });
}

void peer_fold(int dev, hipStream_t s, int op, int dtype, const std::vector<uintptr_t>& srcs, uintptr_t dst, int64_t n,
               int max_blocks) {
  check_fold_args("peer_fold", op, dtype, srcs, {dst});
  if (n <= 0) return;
  with_peer_tag(dtype, [&](auto tag) { launch<decltype(tag)>(dev, s, op, srcs, {dst}, n, true, max_blocks); });
}

}  // namespace mpit
