// The kernels of the window collectives (core/window.cpp Window::pull_gather, scan), one launch
// each between the two barriers of the protocol.
//   peer_gather   dst[g][b] = src[g][b]                      b < bytes[g], up to 8 segments
//   peer_scan     dst[j][i] = src[0][i] op ... op src[j][i]             every j < ns (inclusive)
//                 dst[j][i] = src[0][i] op ... op src[j-1][i]           j >= 1 (exclusive)
// (peer_fold, Window::pull_fold's kernel, is peer_reduce with one destination: allreduce.hip.)
// The sources are usually other members' IPC mappings, at whatever base sym_register exposed
// them: nothing in here assumes that the pointers of a call share their offset within 16 B.
//
// Design (the rules of peer_stream.h, whose skeleton peer_scan runs on): streaming, HBM/xGMI-bound
// kernels; 256-thread blocks; each lane moves 16 B per pointer per step and all loads of a step
// are issued before the first combine or store; the pointer table travels by value in the kernel
// arguments. The vector body is cut so that the destination (peer_gather: one per segment;
// peer_scan: the first one written) is 16-B aligned; every other pointer is accessed where it
// falls, through load16 / store16 (gfx950 executes a global dwordx4 access at any byte
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
#include "peer_ops.h"     // the element tags, widen / narrow / comb, PeerTable, fold: the all-reduce's bits
#include "peer_stream.h"  // the streaming skeleton, load16 / store16, narrow_acc, the launcher

// plain IEEE operations in the stated order: no contraction anywhere in this file
#pragma clang fp contract(off)

namespace mpit {
namespace {

constexpr int kCB = kPeerBlock;
constexpr int kGU = 4;  // peer_gather: vectors per lane per tile (16 KiB per tile)

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
  with_peer_op<Tag>(op, [&](auto o) { scan_chain<Tag, decltype(o)::value, NS, VE>(e, ns, excl, put); });
}

constexpr int scan_u(int NS) { return NS >= 8 ? 1 : 2; }

// the body's vector v is 16-B aligned in the first destination written; every other pointer is accessed where it falls
template <class Tag, int NS>
__global__ __launch_bounds__(kCB) void peer_scan_kernel(PeerTable tab, int op, int excl, int64_t n, int64_t head,
                                                        int64_t nvec) {
  using S = typename Tag::S;
  peer_stream<Tag, NS, scan_u(NS)>(tab, n, head, nvec, [&](int64_t i, const auto& e) {
    scan_op<Tag>(op, e, tab.ns, excl != 0,
                 [&](int k, const auto& o) { put_elems(reinterpret_cast<S*>(tab.dst[k]) + i, o); });
  });
}

// ------------------------------------------------------------------ host twin and launcher
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

template <class Tag>
void launch_scan(int dev, hipStream_t s, int op, bool excl, const std::vector<uintptr_t>& srcs,
                 const std::vector<uintptr_t>& dsts, int64_t n, int max_blocks) {
  using S = typename Tag::S;
  if (dev < 0) {
    host_scan<Tag>(op, excl, srcs, dsts, n);
    return;
  }
  const PeerTable tab = peer_table(srcs, dsts);
  if (excl && tab.ns == 1) return;  // dst[0] is never written
  int64_t head, nvec;
  cut<S>(dsts[excl ? 1 : 0], n, &head, &nvec);  // the first destination written
  peer_launch<S>(dev, "peer_scan launch", tab.ns, n, nvec, max_blocks, scan_u, [&](auto NS, dim3 grid) {
    hipLaunchKernelGGL((peer_scan_kernel<Tag, decltype(NS)::value>), grid, dim3(kCB), 0, s, tab, op, excl ? 1 : 0, n,
                       head, nvec);
  });
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
