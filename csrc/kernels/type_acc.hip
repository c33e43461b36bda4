// One-sided accumulate on a derived-datatype layout in ONE launch (MPI_Accumulate,
// MPI_Get_accumulate, MPI_Fetch_and_op): for every element e of the layout
//     old = strided[e];  strided[e] = comb(op, old, packed[e]);  fetch[e] = old (with a fetch stream)
// where `strided` is the target (a peer's IPC-mapped window), `packed` the origin's contiguous
// stream and `fetch` a contiguous stream of the same size. The layout, the item size (`unit`
// bytes = unit / sizeof(element) elements, so unit >= sizeof(element)), the three run modes, the
// LDS staging of the run table, the index widths and the capped, grid-striding launch are
// type_copy's (type_layout.h). comb / widen / narrow are the all-reduce's (peer_ops.h): the same
// operands give the same bits in Accumulate and Allreduce.
//
// A lane loads its strided and its packed items for all kPerThread slots first, then combines,
// then stores: 16 B per lane and stream when the layout allows. A pair type (MAXLOC / MINLOC) is
// one more element type whose element is the whole pair: an item holds whole pairs, so the layout
// must give unit >= the pair's size. The op is wave-uniform and
// switched once per item. REPLACE stores the origin element and reads the target only for a
// fetch; NO_OP stores nothing and never reads the origin (which may be absent).
// There are NO atomics in here: mutual exclusion is the target window's exclusive lock
// (Window::accumulate_plan). Overlapping target runs are erroneous and undefined.
#include <cstring>
#include <stdexcept>
#include <string>

#include "kernels.h"
#include "ew.h"
#include "peer_ops.h"
#include "type_layout.h"

// plain IEEE operations in the stated order: no contraction anywhere in this file
#pragma clang fp contract(off)

namespace mpit {
namespace {

using namespace tl;

struct TaArgs {
  uint8_t* strided;
  const uint8_t* packed;
  uint8_t* fetch;
  Layout lay;
  int op;
};

template <class Tag, int OP, int VE>
MPIT_HD void comb_all(const typename Tag::S (&t)[VE], const typename Tag::S (&o)[VE], typename Tag::S (&r)[VE]) {
#pragma unroll
  for (int e = 0; e < VE; ++e) r[e] = narrow<Tag>(comb<Tag, OP>(widen<Tag>(t[e]), widen<Tag>(o[e])));
}

// r = comb(op, t, o) element by element; op is one of the ten PeerOp (REPLACE / NO_OP are the caller's)
template <class Tag, int VE>
MPIT_HD void comb_op(int op, const typename Tag::S (&t)[VE], const typename Tag::S (&o)[VE],
                     typename Tag::S (&r)[VE]) {
  with_peer_op<Tag>(op, [&](auto c) { comb_all<Tag, decltype(c)::value, VE>(t, o, r); });
}

template <class Tag, typename V, typename IT, int MODE>
__global__ __launch_bounds__(kTB) void type_acc_kernel(TaArgs a) {
  using S = typename Tag::S;
  constexpr int VE = int(sizeof(V) / sizeof(S));
  static_assert(VE >= 1 && sizeof(V) == VE * sizeof(S), "an item holds whole elements");
  __shared__ int64_t sh[lds_words<MODE>()];
  const int64_t *offs, *pre;
  stage_table<MODE>(a.lay, sh, offs, pre);
  const int op = a.op;
  const bool ld_old = a.fetch != nullptr || op != kAccReplace;  // all three are grid-uniform
  const bool ld_org = op != kAccNoOp;
  const bool st_new = op != kAccNoOp;
  const int64_t step = int64_t(gridDim.x) * kTile;
  for (int64_t t0 = int64_t(blockIdx.x) * kTile; t0 < a.lay.items; t0 += step) {
    V told[kPerThread], torg[kPerThread];
    uint8_t* sp[kPerThread];
    int64_t pq[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const int64_t i = t0 + j * kTB + threadIdx.x;
      sp[j] = nullptr;
      pq[j] = 0;
      told[j] = V(0);
      torg[j] = V(0);
      if (i < a.lay.items) {
        const IT q = IT(i) * IT(sizeof(V));
        sp[j] = a.strided + strided_offset<IT, MODE>(a.lay, offs, pre, q);
        pq[j] = int64_t(q);
        if (ld_old) told[j] = *reinterpret_cast<const V*>(sp[j]);
        if (ld_org) torg[j] = *reinterpret_cast<const V*>(a.packed + pq[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      if (!sp[j]) continue;
      if (st_new) {
        V out = torg[j];
        if (op != kAccReplace) {
          S t[VE], o[VE], r[VE];
          __builtin_memcpy(t, &told[j], sizeof(V));
          __builtin_memcpy(o, &torg[j], sizeof(V));
          __builtin_memcpy(r, &told[j], sizeof(V));
          comb_op<Tag, VE>(op, t, o, r);
          __builtin_memcpy(&out, r, sizeof(V));
        }
        *reinterpret_cast<V*>(sp[j]) = out;
      }
      if (a.fetch) *reinterpret_cast<V*>(a.fetch + pq[j]) = told[j];
    }
  }
}

template <class Tag, typename V, typename IT>
void launch_mode(int mode, dim3 grid, hipStream_t s, const TaArgs& a) {
  if (mode == 0) hipLaunchKernelGGL((type_acc_kernel<Tag, V, IT, 0>), grid, dim3(kTB), 0, s, a);
  else if (mode == 1) hipLaunchKernelGGL((type_acc_kernel<Tag, V, IT, 1>), grid, dim3(kTB), 0, s, a);
  else hipLaunchKernelGGL((type_acc_kernel<Tag, V, IT, 2>), grid, dim3(kTB), 0, s, a);
}

// unit < sizeof(element) was refused by the caller: those items are never instantiated
template <class Tag, typename V>
void launch_unit(bool wide, int mode, dim3 grid, hipStream_t s, const TaArgs& a) {
  if constexpr (sizeof(V) >= sizeof(typename Tag::S)) {
    if (wide) launch_mode<Tag, V, uint64_t>(mode, grid, s, a);
    else launch_mode<Tag, V, uint32_t>(mode, grid, s, a);
  }
}

template <class Tag>
void host_acc(const TaArgs& a, const tl::Checked& c, const int64_t* offs, const int64_t* pre) {
  using S = typename Tag::S;
  const int op = a.op;
  const S* pp = reinterpret_cast<const S*>(a.packed);
  S* fp = reinterpret_cast<S*>(a.fetch);
  for (int64_t i0 = 0; i0 < c.n[0]; ++i0)
    for (int64_t i1 = 0; i1 < c.n[1]; ++i1)
      for (int64_t i2 = 0; i2 < c.n[2]; ++i2) {
        uint8_t* base = a.strided + i0 * c.st[0] + i1 * c.st[1] + i2 * c.st[2];
        for (int64_t r = 0; r < a.lay.R; ++r) {
          const int64_t len = a.lay.L ? a.lay.L : pre[r + 1] - pre[r];
          S* sp = reinterpret_cast<S*>(base + (offs ? offs[r] : 0));
          const int64_t ne = len / int64_t(sizeof(S));
          for (int64_t e = 0; e < ne; ++e) {
            S t[1] = {sp[e]}, o[1] = {op != kAccNoOp ? pp[e] : S{}}, res[1] = {t[0]};
            if (op == kAccReplace) sp[e] = o[0];
            else if (op != kAccNoOp) {
              comb_op<Tag, 1>(op, t, o, res);
              sp[e] = res[0];
            }
            if (fp) fp[e] = t[0];
          }
          pp += ne;
          if (fp) fp += ne;
        }
      }
}

template <class Tag>
void run(int dev, hipStream_t s, const TaArgs& a, const tl::Checked& c, int unit, int mode, dim3 grid, bool wide) {
  if (dev < 0) {
    const int64_t* offs = a.lay.table;
    host_acc<Tag>(a, c, offs, offs ? offs + a.lay.R : nullptr);
    return;
  }
  hip_check(hipSetDevice(dev), "hipSetDevice");
  switch (unit) {
    case 16: launch_unit<Tag, u32x4>(wide, mode, grid, s, a); break;
    case 8: launch_unit<Tag, u32x2>(wide, mode, grid, s, a); break;
    case 4: launch_unit<Tag, uint32_t>(wide, mode, grid, s, a); break;
    case 2: launch_unit<Tag, uint16_t>(wide, mode, grid, s, a); break;
    default: launch_unit<Tag, uint8_t>(wide, mode, grid, s, a); break;
  }
  hip_check(hipGetLastError(), "type_accumulate launch");
}

void bad(const std::string& what) { throw std::invalid_argument("mpit: type_accumulate: " + what); }

}  // namespace

bool type_accumulate_supported(int op, int dtype) {
  if (peer_dtype_is_pair(dtype)) return peer_reduce_supported(op, dtype);  // the two pair ops and nothing else
  if (dtype < 0 || dtype >= kPrDtypes) return false;
  return op == kAccReplace || op == kAccNoOp || peer_reduce_supported(op, dtype);
}

void type_accumulate(int dev, hipStream_t s, int op, int dtype, uintptr_t strided, uintptr_t packed, uintptr_t fetch,
                     const std::vector<std::array<int64_t, 2>>& loops, uintptr_t table, int64_t R, int64_t L,
                     int64_t per, int unit, int max_blocks, bool wide) {
  if (!type_accumulate_supported(op, dtype)) bad("unsupported (op, dtype)");
  const int es = peer_dtype_size(dtype);
  if (!strided) bad("null target");
  if (!packed && op != kAccNoOp) bad("an origin stream is needed unless the op is NO_OP");
  const tl::Checked c = tl::check_layout("type_accumulate", strided, packed, loops, table, R, L, per, unit);
  if (unit < es)
    bad(peer_dtype_is_pair(dtype) ? "unit " + std::to_string(unit) + " is smaller than the pair of " +
                                        std::to_string(es) + " bytes"
                                  : std::string("unit is smaller than the element"));
  if (fetch % uintptr_t(unit)) bad("unit does not divide the layout");
  if (c.bytes == 0) return;
  if (op == kAccNoOp && !fetch) return;  // nothing to store anywhere
  TaArgs a;
  a.strided = reinterpret_cast<uint8_t*>(strided);
  a.packed = reinterpret_cast<const uint8_t*>(packed);
  a.fetch = reinterpret_cast<uint8_t*>(fetch);
  a.lay = tl::make_layout(c, table, R, L, per, unit);
  a.op = op;
  const int mode = tl::layout_mode(table, R, L);
  wide = wide || c.bytes >= (int64_t(1) << 32);
  const dim3 grid = tl::layout_grid(a.lay.items, max_blocks);
  with_peer_tag(dtype, [&](auto tag) { run<decltype(tag)>(dev, s, a, c, unit, mode, grid, wide); });
}

}  // namespace mpit
