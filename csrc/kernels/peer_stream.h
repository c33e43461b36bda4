// The frame of the peer kernels that read element i of up to 8 sources and write it somewhere
// (allreduce.hip: peer_reduce, peer_fold; peer_coll.hip: peer_scan). peer_scan runs on the
// skeleton; peer_reduce_kernel keeps the same frame spelled out, because on the skeleton ten of
// its instances took more registers than before (allreduce.hip), and uses the rest of this header:
//   peer_stream    the device skeleton: tile loop, load phase, scalar head and tail
//   load16/store16 every 16-byte access, where it falls
//   narrow_acc     what every reducing kernel narrows with
//   cut, grid_for, check_fold_args, peer_launch    the host side of a launch
// Rules (cdna_hip_programming.md Guideline 13, Appendix "Element-wise"): streaming, HBM/xGMI-bound
// kernels; 256-thread blocks; each lane moves 16 B per source per step and all NS x U loads of a
// tile are issued before the body runs on the first of them. NS is a template parameter in
// {1, 2, 4, 8}: a source count in between re-loads the last source (an L2 hit) and the body skips
// it, so no load hides behind a runtime condition. Elements [0, head) and [head + nvec*VE, n) run
// scalar, spread over the grid; vector v of the body is elements [head + v*VE, head + (v+1)*VE).
// Where the body is cut is the entry point's business (cut); every 16-byte access is made where
// it falls (gfx950 executes a global dwordx4 access at any byte address; a second cache line per
// access at most), so no pointer need share its offset within 16 B with another.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "ew.h"
#include "kernels.h"
#include "peer_ops.h"

namespace mpit {

constexpr int kPeerBlock = 256;
constexpr int kPeerGrid = 2048;  // the production cap of the grid (max_blocks == 0)

MPIT_HD uint4 load16(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
MPIT_HD void store16(uint8_t* p, const uint4& v) { __builtin_memcpy(p, &v, 16); }

// o[0..VE) to p: one 16-byte store where it falls, or one element
template <class S, int VE>
MPIT_HD void put_elems(S* p, const S (&o)[VE]) {
  if constexpr (VE * sizeof(S) == 16) {
    uint4 out;
    __builtin_memcpy(&out, o, 16);
    store16(reinterpret_cast<uint8_t*>(p), out);
  } else {
    *p = o[0];
  }
}

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

// body(i, e): e[k][0..VE) are elements [i, i + VE) of source k, for every k < NS (k >= tab.ns
// repeats the last source). VE = 16 / sizeof(S) in the tile loop and 1 in the scalar loop.
// In place: a lane has loaded every element it owns before the body stores any of them, and no
// two lanes own the same element, so a destination may be a source.
template <class Tag, int NS, int U, class Body>
__device__ __forceinline__ void peer_stream(const PeerTable& tab, int64_t n, int64_t head, int64_t nvec,
                                            Body&& body) {
  using S = typename Tag::S;
  constexpr int VE = 16 / int(sizeof(S));
  const int ns = tab.ns;
  auto src = [&](int k) { return reinterpret_cast<const S*>(tab.src[k < ns ? k : ns - 1]); };
  const int64_t tile = int64_t(kPeerBlock) * U;
  const int64_t ntiles = (nvec + tile - 1) / tile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint4 raw[U][NS];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kPeerBlock + threadIdx.x;
      if (v < nvec) {
#pragma unroll
        for (int k = 0; k < NS; ++k) raw[u][k] = load16(reinterpret_cast<const uint8_t*>(src(k) + head + v * VE));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = t * tile + u * kPeerBlock + threadIdx.x;
      if (v < nvec) {
        S e[NS][VE];
#pragma unroll
        for (int k = 0; k < NS; ++k) __builtin_memcpy(e[k], &raw[u][k], 16);
        body(head + v * VE, e);
      }
    }
  }
  const int64_t tail0 = head + nvec * VE;
  const int64_t nsc = head + (n - tail0);
  for (int64_t q = int64_t(blockIdx.x) * kPeerBlock + threadIdx.x; q < nsc; q += int64_t(gridDim.x) * kPeerBlock) {
    const int64_t i = q < head ? q : tail0 + (q - head);
    S e[NS][1];
#pragma unroll
    for (int k = 0; k < NS; ++k) e[k][0] = src(k)[i];
    body(i, e);
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

inline unsigned grid_for(int64_t want, int max_blocks) {
  const int64_t cap = max_blocks > 0 ? max_blocks : kPeerGrid;
  return unsigned(std::max<int64_t>(1, std::min<int64_t>(want, cap)));
}

// count_dsts: the caller's destinations are a list of their own (peer_reduce), 1..8 like the sources
inline void check_fold_args(const char* who, int op, int dtype, const std::vector<uintptr_t>& srcs,
                            const std::vector<uintptr_t>& dsts, bool count_dsts = false) {
  const std::string w(who);
  if (!peer_reduce_supported(op, dtype)) throw std::invalid_argument(w + ": unsupported (op, dtype)");
  if (srcs.empty() || srcs.size() > size_t(kPeerMax) ||
      (count_dsts && (dsts.empty() || dsts.size() > size_t(kPeerMax))))
    throw std::invalid_argument(w + (count_dsts ? ": 1..8 sources and destinations" : ": 1..8 sources"));
  const uintptr_t es = uintptr_t(peer_dtype_align(dtype));
  for (uintptr_t p : srcs)
    if (!p || p % es) throw std::invalid_argument(w + ": null or misaligned source");
  for (uintptr_t p : dsts)
    if (!p || p % es) throw std::invalid_argument(w + ": null or misaligned destination");
}

inline PeerTable peer_table(const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts) {
  PeerTable tab{};
  tab.ns = int32_t(srcs.size());
  tab.nd = int32_t(dsts.size());
  std::copy(srcs.begin(), srcs.end(), tab.src);
  std::copy(dsts.begin(), dsts.end(), tab.dst);
  return tab;
}

// One launch of a peer_stream kernel: picks NS in {1, 2, 4, 8} for ns sources, sizes the grid for
// u_of(NS) vectors per lane and the scalar part, and calls launch(integral_constant<int, NS>, grid).
template <class S, class Launch>
void peer_launch(int dev, const char* what, int ns, int64_t n, int64_t nvec, int max_blocks, int (*u_of)(int),
                 Launch&& launch) {
  constexpr int VE = 16 / int(sizeof(S));
  const int NS = ns <= 1 ? 1 : (ns <= 2 ? 2 : (ns <= 4 ? 4 : 8));
  const int64_t tile = int64_t(kPeerBlock) * u_of(NS);
  const int64_t nsc = n - nvec * VE;
  const dim3 grid(grid_for(std::max((nvec + tile - 1) / tile, (nsc + kPeerBlock - 1) / kPeerBlock), max_blocks));
  hip_check(hipSetDevice(dev), "hipSetDevice");
  switch (NS) {
    case 1: launch(std::integral_constant<int, 1>{}, grid); break;
    case 2: launch(std::integral_constant<int, 2>{}, grid); break;
    case 4: launch(std::integral_constant<int, 4>{}, grid); break;
    default: launch(std::integral_constant<int, 8>{}, grid); break;
  }
  hip_check(hipGetLastError(), what);
}

}  // namespace mpit
