// The layout walk shared by the derived-datatype kernels (type_copy.hip, type_acc.hip): the
// launch geometry, the layout as a kernel argument, the run-table staging, the packed byte ->
// strided byte offset mapping and the host-side argument checks. See type_copy.hip for the
// layout's definition.
#pragma once
#include <algorithm>
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "ew.h"
#include "kernels.h"

namespace mpit {
namespace tl {

constexpr int kTB = 256;
constexpr int kPerThread = 4;
constexpr int64_t kTile = int64_t(kTB) * kPerThread;
constexpr int kLdsRuns = 1024;
constexpr int kMaxBlocks = 2048;

// plain clang vectors: an array of them stays in registers (HIP's uint4 wrapper class went to scratch)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Layout {
  const int64_t* table;
  int64_t n1, n2;  // the two inner loop counts (the outermost is implied by `items`)
  int64_t s0, s1, s2;
  int64_t R, L, per;  // per = packed bytes of one innermost iteration
  int64_t items;
  int lds;
};

// MODE 0: one run at offset 0; 1: equal-length runs; 2: prefix-sum search
template <int MODE>
constexpr int lds_words() { return MODE == 0 ? 1 : 2 * kLdsRuns + 1; }

// offs / pre of the block: the table in global memory, or its copy in `sh` when it fits
template <int MODE>
__device__ __forceinline__ void stage_table(const Layout& a, int64_t* sh, const int64_t*& offs, const int64_t*& pre) {
  offs = a.table;
  pre = a.table + a.R;
  if (MODE != 0 && a.lds) {
    const int nw = int(MODE == 1 ? a.R : 2 * a.R + 1);
    for (int i = threadIdx.x; i < nw; i += kTB) sh[i] = a.table[i];
    __syncthreads();
    offs = sh;
    pre = sh + a.R;
  }
}

// the strided byte offset of packed byte q (the first byte of an item, which never straddles a run)
template <typename IT, int MODE>
__device__ __forceinline__ int64_t strided_offset(const Layout& a, const int64_t* offs, const int64_t* pre, IT q) {
  const IT per = IT(a.per), L = IT(a.L), n1 = IT(a.n1), n2 = IT(a.n2);
  IT it = q / per;
  IT rem = q - it * per;
  const IT i2 = it % n2;
  it /= n2;
  const IT i1 = it % n1;
  const IT i0 = it / n1;
  int64_t off = int64_t(i0) * a.s0 + int64_t(i1) * a.s1 + int64_t(i2) * a.s2;
  if (MODE == 1) {
    const IT r = rem / L;
    rem -= r * L;
    off += offs[r];
  } else if (MODE == 2) {
    int lo = 0, hi = int(a.R);
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (IT(pre[mid]) <= rem) lo = mid;
      else hi = mid;
    }
    rem -= IT(pre[lo]);
    off += offs[lo];
  }
  return off + int64_t(rem);
}

// The checks every entry point makes on (loops, table, R, L, per, unit) and two base addresses:
// std::invalid_argument in the name of `who`, else the loops right-aligned in n / st and the
// packed size in bytes (0: nothing to move).
struct Checked {
  int64_t n[3] = {1, 1, 1}, st[3] = {0, 0, 0};
  int64_t bytes = 0;
};

inline Checked check_layout(const char* who, uintptr_t strided, uintptr_t packed,
                            const std::vector<std::array<int64_t, 2>>& loops, uintptr_t table, int64_t R, int64_t L,
                            int64_t per, int unit) {
  auto bad = [&](const char* what) { throw std::invalid_argument(std::string("mpit: ") + who + ": " + what); };
  if (loops.size() > 3) bad("at most three loops");
  if (unit != 1 && unit != 2 && unit != 4 && unit != 8 && unit != 16) bad("unit is a power of two <= 16");
  if (R < 1 || L < 0 || per <= 0) bad("R >= 1, L >= 0 and per > 0");
  if (L != 0 && per != R * L) bad("per != R * L");
  if (!table && !(R == 1 && L != 0)) bad("a run table is needed unless R == 1 with L != 0");
  if (per % unit || L % unit || strided % uintptr_t(unit) || packed % uintptr_t(unit)) bad("unit does not divide the layout");
  Checked c;
  unsigned __int128 total = uint64_t(per);
  for (size_t k = 0; k < loops.size(); ++k) {
    const size_t at = 3 - loops.size() + k;
    c.n[at] = loops[k][0];
    c.st[at] = loops[k][1];
    if (c.n[at] < 0) bad("negative loop count");
    if (c.n[at] > 1 && c.st[at] % unit) bad("unit does not divide a loop stride");
    total *= uint64_t(c.n[at]);
    if (total >> 62) bad("packed size overflows");
  }
  c.bytes = int64_t(total);
  return c;
}

inline Layout make_layout(const Checked& c, uintptr_t table, int64_t R, int64_t L, int64_t per, int unit) {
  Layout a;
  a.table = reinterpret_cast<const int64_t*>(table);
  a.n1 = c.n[1];
  a.n2 = c.n[2];
  a.s0 = c.st[0];
  a.s1 = c.st[1];
  a.s2 = c.st[2];
  a.R = R;
  a.L = L;
  a.per = per;
  a.items = c.bytes / unit;
  a.lds = R <= kLdsRuns;
  return a;
}

inline int layout_mode(uintptr_t table, int64_t R, int64_t L) { return L == 0 ? 2 : (R == 1 && !table ? 0 : 1); }

inline dim3 layout_grid(int64_t items, int max_blocks) {
  int64_t cap = kMaxBlocks;
  if (max_blocks > 0) cap = std::min<int64_t>(cap, max_blocks);
  return dim3(unsigned(std::min<int64_t>((items + kTile - 1) / kTile, cap)));
}

}  // namespace tl
}  // namespace mpit
