// peer_plan_gather: up to 8 independent layout-to-layout copies in ONE launch, the kernel of the
// irregular window collectives (core/window.cpp Window::pull_plan: Gatherv, Scatterv, Alltoallv
// and the strided Alltoallw). Segment g has a source side and a destination side, each a base
// address plus a layout exactly as type_copy.hip defines it (up to three loops around a table of
// R runs, packed order loops outermost to innermost, runs in table order, ascending bytes); a
// contiguous side is the one-run layout. For every packed byte q of segment g
//     dst_g[off_dst(q)] = src_g[off_src(q)].
// The sources are usually other members' IPC mappings; the destinations are local.
//
// Design (the rules of peer_coll.hip and type_copy.hip): 256-thread blocks, kPerThread items per
// thread and round, all loads of a round before its first store; one item = the segment's `unit`
// bytes (the largest power of two <= 16 dividing every offset, length, stride and base address
// of both sides), so no item straddles a run on either side and every access is naturally
// aligned. The grid is capped and strides over the tiles of all segments together: a block
// finds the segment of a tile in a prefix table of per-segment tile counts (a wave-uniform scan
// of at most 8 entries), so a 3-byte segment and a long one share one grid. The segment
// descriptors (two tl::Layout each) travel by value in the kernel arguments, 1.8 KiB of them.
// Both sides walk through tl::strided_offset in one of the three run modes of type_layout.h,
// chosen per side and segment at run time (wave-uniform branches). Run tables are staged in LDS
// when R <= tl::kLdsRuns (1,024 runs, 16 KiB per side) and read from global memory above that; a
// block whose grid-stride loop passes into another segment stages that segment's tables anew
// behind a barrier. Index arithmetic is 32-bit while every segment packs below 4 GiB and 64-bit
// otherwise (or when `wide` is set); byte offsets are always 64-bit. Plain vector loads and
// stores only: no atomics, no cross-rank flags, no spinning on peer memory.
#include <cstring>
#include <stdexcept>
#include <string>

#include "ew.h"
#include "kernels.h"
#include "type_layout.h"

namespace mpit {
namespace {

using namespace tl;

struct PlanSegArgs {
  const uint8_t* src;
  uint8_t* dst;
  Layout s, d;  // (s.items == d.items: the segment's items of `unit` bytes)
  int32_t unit, smode, dmode, pad;
};

struct PlanArgs {
  PlanSegArgs seg[kPeerMax];
  int64_t tiles[kPeerMax];  // inclusive prefix of the per-segment tile counts
  int32_t ng;
};
static_assert(sizeof(PlanArgs) <= 4096, "the descriptors must fit the kernel argument segment");

// the table of one side for this block (tl::stage_table in the side's run mode)
__device__ __forceinline__ void stage_side(int mode, const Layout& a, int64_t* sh, const int64_t*& offs,
                                           const int64_t*& pre) {
  if (mode == 1) stage_table<1>(a, sh, offs, pre);
  else if (mode == 2) stage_table<2>(a, sh, offs, pre);
  else stage_table<0>(a, sh, offs, pre);
}

// byte offsets of this thread's kPerThread items of the tile at item t0 (valid items only)
template <typename IT, int MODE>
__device__ __forceinline__ void side_offsets(const Layout& a, const int64_t* offs, const int64_t* pre, int64_t t0,
                                             int unit, int64_t (&out)[kPerThread]) {
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t i = t0 + j * kTB + threadIdx.x;
    if (i < a.items) out[j] = strided_offset<IT, MODE>(a, offs, pre, IT(i) * IT(unit));
  }
}

template <typename IT>
__device__ __forceinline__ void side_offsets_mode(int mode, const Layout& a, const int64_t* offs, const int64_t* pre,
                                                  int64_t t0, int unit, int64_t (&out)[kPerThread]) {
  if (mode == 1) side_offsets<IT, 1>(a, offs, pre, t0, unit, out);
  else if (mode == 2) side_offsets<IT, 2>(a, offs, pre, t0, unit, out);
  else side_offsets<IT, 0>(a, offs, pre, t0, unit, out);
}

template <typename V>
__device__ __forceinline__ void move_items(const uint8_t* src, uint8_t* dst, const int64_t (&so)[kPerThread],
                                           const int64_t (&dof)[kPerThread], int64_t t0, int64_t items) {
  V v[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (t0 + j * kTB + threadIdx.x < items) v[j] = *reinterpret_cast<const V*>(src + so[j]);
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (t0 + j * kTB + threadIdx.x < items) *reinterpret_cast<V*>(dst + dof[j]) = v[j];
}

template <typename IT>
__global__ __launch_bounds__(kTB) void peer_plan_kernel(PlanArgs a) {
  __shared__ int64_t sh_s[lds_words<2>()];
  __shared__ int64_t sh_d[lds_words<2>()];
  const int ng = a.ng;
  const int64_t total = a.tiles[ng - 1];
  const int64_t *soffs = nullptr, *spre = nullptr, *doffs = nullptr, *dpre = nullptr;
  int staged = -1;  // the segment whose tables this block holds
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    int g = 0;
    while (g < ng - 1 && t >= a.tiles[g]) ++g;  // wave-uniform, at most 7 steps
    const PlanSegArgs& sg = a.seg[g];
    if (g != staged) {
      if (staged >= 0) __syncthreads();  // every wave has finished with the previous segment's tables
      stage_side(sg.smode, sg.s, sh_s, soffs, spre);
      stage_side(sg.dmode, sg.d, sh_d, doffs, dpre);
      staged = g;
    }
    const int64_t t0 = (t - (g ? a.tiles[g - 1] : 0)) * kTile;
    const int unit = sg.unit;
    int64_t so[kPerThread], dof[kPerThread];
    side_offsets_mode<IT>(sg.smode, sg.s, soffs, spre, t0, unit, so);
    side_offsets_mode<IT>(sg.dmode, sg.d, doffs, dpre, t0, unit, dof);
    const int64_t items = sg.s.items;
    switch (unit) {
      case 16: move_items<u32x4>(sg.src, sg.dst, so, dof, t0, items); break;
      case 8: move_items<u32x2>(sg.src, sg.dst, so, dof, t0, items); break;
      case 4: move_items<uint32_t>(sg.src, sg.dst, so, dof, t0, items); break;
      case 2: move_items<uint16_t>(sg.src, sg.dst, so, dof, t0, items); break;
      default: move_items<uint8_t>(sg.src, sg.dst, so, dof, t0, items); break;
    }
  }
}

void bad(const std::string& what) { throw std::invalid_argument("mpit: peer_plan_gather: " + what); }

// one side after the checks: the loops right-aligned, the packed size
struct Side {
  Checked c;
  const PlanSide* p;
};

struct Live {  // a segment with something to move
  Side s, d;
  int unit;
};

bool same_side(const Side& a, const Side& b) {
  if (a.p->base != b.p->base || a.p->table != b.p->table || a.p->R != b.p->R || a.p->L != b.p->L || a.p->per != b.p->per)
    return false;
  for (int k = 0; k < 3; ++k)
    if (a.c.n[k] != b.c.n[k] || (a.c.n[k] > 1 && a.c.st[k] != b.c.st[k])) return false;
  return true;
}

// The runs of a side in packed order, for the host twin.
struct RunWalk {
  const Side& s;
  const int64_t* offs;
  const int64_t* pre;
  int64_t i0 = 0, i1 = 0, i2 = 0, r = 0, done = 0;  // done: bytes of the current run already consumed
  explicit RunWalk(const Side& side)
      : s(side), offs(reinterpret_cast<const int64_t*>(side.p->table)), pre(offs ? offs + side.p->R : nullptr) {}
  int64_t len() const { return (s.p->L ? s.p->L : pre[r + 1] - pre[r]) - done; }
  uint8_t* at() const {
    return reinterpret_cast<uint8_t*>(s.p->base) + i0 * s.c.st[0] + i1 * s.c.st[1] + i2 * s.c.st[2] +
           (offs ? offs[r] : 0) + done;
  }
  void advance(int64_t n) {
    done += n;
    if (len() > 0) return;
    done = 0;
    if (++r < s.p->R) return;
    r = 0;
    if (++i2 < s.c.n[2]) return;
    i2 = 0;
    if (++i1 < s.c.n[1]) return;
    i1 = 0;
    ++i0;
  }
};

void host_segment(const Side& src, const Side& dst) {
  RunWalk a(src), b(dst);
  for (int64_t left = src.c.bytes; left > 0;) {
    while (a.len() == 0) a.advance(0);  // (a zero-length run of an irregular table)
    while (b.len() == 0) b.advance(0);
    const int64_t n = std::min(a.len(), b.len());
    std::memcpy(b.at(), a.at(), size_t(n));
    a.advance(n);
    b.advance(n);
    left -= n;
  }
}

// The checks of every segment; the live ones (not empty, not a copy onto itself) in their order.
std::vector<Live> checked_segments(const std::vector<PlanSegment>& segs) {
  if (segs.size() > size_t(kPeerMax)) bad("up to 8 segments");
  std::vector<Live> live;
  for (const PlanSegment& g : segs) {
    Side s{check_layout("peer_plan_gather", g.src.base, g.src.base, g.src.loops, g.src.table, g.src.R, g.src.L,
                        g.src.per, g.unit),
           &g.src};
    Side d{check_layout("peer_plan_gather", g.dst.base, g.dst.base, g.dst.loops, g.dst.table, g.dst.R, g.dst.L,
                        g.dst.per, g.unit),
           &g.dst};
    if (s.c.bytes != d.c.bytes) bad("the two sides of a segment differ in packed size");
    if (s.c.bytes == 0 || same_side(s, d)) continue;  // nothing to move
    if (!g.src.base || !g.dst.base) bad("null source or destination");
    live.push_back({s, d, g.unit});
  }
  return live;
}

}  // namespace

void peer_plan_check(const std::vector<PlanSegment>& segs) { (void)checked_segments(segs); }

void peer_plan_gather(int dev, hipStream_t s, const std::vector<PlanSegment>& segs, int max_blocks, bool wide) {
  const std::vector<Live> live = checked_segments(segs);
  if (live.empty()) return;
  if (dev < 0) {
    for (const Live& v : live) host_segment(v.s, v.d);
    return;
  }
  PlanArgs a{};
  int64_t total = 0;
  int ng = 0;
  for (const Live& v : live) {
    PlanSegArgs& g = a.seg[ng];
    g.src = reinterpret_cast<const uint8_t*>(v.s.p->base);
    g.dst = reinterpret_cast<uint8_t*>(v.d.p->base);
    g.s = make_layout(v.s.c, v.s.p->table, v.s.p->R, v.s.p->L, v.s.p->per, v.unit);
    g.d = make_layout(v.d.c, v.d.p->table, v.d.p->R, v.d.p->L, v.d.p->per, v.unit);
    g.unit = v.unit;
    g.smode = layout_mode(v.s.p->table, v.s.p->R, v.s.p->L);
    g.dmode = layout_mode(v.d.p->table, v.d.p->R, v.d.p->L);
    wide = wide || v.s.c.bytes >= (int64_t(1) << 32);
    total += (g.s.items + kTile - 1) / kTile;
    a.tiles[ng] = total;
    ++ng;
  }
  a.ng = ng;
  int64_t cap = kMaxBlocks;
  if (max_blocks > 0) cap = std::min<int64_t>(cap, max_blocks);
  const dim3 grid(unsigned(std::min<int64_t>(total, cap)));
  hip_check(hipSetDevice(dev), "hipSetDevice");
  if (wide) hipLaunchKernelGGL((peer_plan_kernel<uint64_t>), grid, dim3(kTB), 0, s, a);
  else hipLaunchKernelGGL((peer_plan_kernel<uint32_t>), grid, dim3(kTB), 0, s, a);
  hip_check(hipGetLastError(), "peer_plan_gather launch");
}

}  // namespace mpit
