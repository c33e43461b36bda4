// Derived-datatype pack / unpack: a strided byte layout <-> one contiguous packed stream in ONE
// launch (MPI_Pack / MPI_Unpack, the packing of a derived-type Send / Recv and the strided side
// of a derived-type Put / Get, where `strided` is a peer's IPC-mapped window).
//
// The layout is a plan (mpit_amd/datatypes.py Plan), never an expanded index: up to three outer
// loops (n_k, stride_k bytes), outermost first, around a table of R runs (byte offset, length).
// The packed stream is the loops outermost to innermost, then the runs in table order, then
// ascending bytes. The table is int64 [offs[R] | prefix[R + 1]] (prefix sums of the lengths);
// with all lengths equal (L != 0) only offs is read, and with R == 1 and no table the run starts
// at offset 0.
//
// One item = `unit` bytes of the packed stream, unit = the largest power of two <= 16 dividing
// every offset, length, stride and both base addresses, so an item never straddles a run and
// every access is naturally aligned: 16 B per lane when the layout allows it. Item -> loop
// indices by division; item -> run by division (L != 0) or by binary search of the prefix sums,
// staged in LDS when R <= kLdsRuns and read from global memory above that. Consecutive lanes
// take consecutive items, so the packed side is always coalesced and the strided side is
// coalesced within a run. Blocks of 256 threads move kPerThread items per thread and round
// (loads first, then stores), the grid is capped and grid-strides the rest. The index
// arithmetic is 32-bit when the packed stream is below 4 GiB and 64-bit otherwise; strided
// byte offsets are always 64-bit.
#include <cstring>
#include <stdexcept>
#include <string>

#include "kernels.h"
#include "ew.h"
#include "type_layout.h"  // the geometry, the layout argument and the item -> address walk (shared with type_acc.hip)

namespace mpit {
namespace {

using namespace tl;

struct TcArgs {
  uint8_t* strided;
  uint8_t* packed;
  Layout lay;
  int dir;  // 0 gather strided -> packed, 1 scatter packed -> strided
};

// MODE 0: one run at offset 0; 1: equal-length runs; 2: prefix-sum search
template <typename V, typename IT, int MODE>
__global__ __launch_bounds__(kTB) void type_copy_kernel(TcArgs a) {
  __shared__ int64_t sh[lds_words<MODE>()];
  const int64_t *offs, *pre;
  stage_table<MODE>(a.lay, sh, offs, pre);
  const int64_t step = int64_t(gridDim.x) * kTile;
  for (int64_t t0 = int64_t(blockIdx.x) * kTile; t0 < a.lay.items; t0 += step) {
    V v[kPerThread];
    uint8_t* dst[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const int64_t i = t0 + j * kTB + threadIdx.x;
      dst[j] = nullptr;
      if (i < a.lay.items) {
        const IT q = IT(i) * IT(sizeof(V));
        uint8_t* sp = a.strided + strided_offset<IT, MODE>(a.lay, offs, pre, q);
        uint8_t* pp = a.packed + int64_t(q);
        v[j] = *reinterpret_cast<const V*>(a.dir ? pp : sp);
        dst[j] = a.dir ? sp : pp;
      }
    }
#pragma unroll
    for (int j = 0; j < kPerThread; ++j)
      if (dst[j]) *reinterpret_cast<V*>(dst[j]) = v[j];
  }
}

template <typename V, typename IT>
void launch_mode(int mode, dim3 grid, hipStream_t s, const TcArgs& a) {
  if (mode == 0) hipLaunchKernelGGL((type_copy_kernel<V, IT, 0>), grid, dim3(kTB), 0, s, a);
  else if (mode == 1) hipLaunchKernelGGL((type_copy_kernel<V, IT, 1>), grid, dim3(kTB), 0, s, a);
  else hipLaunchKernelGGL((type_copy_kernel<V, IT, 2>), grid, dim3(kTB), 0, s, a);
}

template <typename V>
void launch_unit(bool wide, int mode, dim3 grid, hipStream_t s, const TcArgs& a) {
  if (wide) launch_mode<V, uint64_t>(mode, grid, s, a);
  else launch_mode<V, uint32_t>(mode, grid, s, a);
}

void bad(const std::string& what) { throw std::invalid_argument("mpit: type_copy: " + what); }

}  // namespace

void type_copy(int dev, hipStream_t s, int dir, uintptr_t strided, uintptr_t packed,
               const std::vector<std::array<int64_t, 2>>& loops, uintptr_t table, int64_t R, int64_t L, int64_t per,
               int unit, int max_blocks, bool wide) {
  if (dir != 0 && dir != 1) bad("dir is 0 (gather) or 1 (scatter)");
  const Checked c = check_layout("type_copy", strided, packed, loops, table, R, L, per, unit);
  if (c.bytes == 0) return;
  if (dev < 0) {
    const int64_t* offs = reinterpret_cast<const int64_t*>(table);
    const int64_t* pre = offs ? offs + R : nullptr;
    uint8_t* sb = reinterpret_cast<uint8_t*>(strided);
    uint8_t* pp = reinterpret_cast<uint8_t*>(packed);
    for (int64_t i0 = 0; i0 < c.n[0]; ++i0)
      for (int64_t i1 = 0; i1 < c.n[1]; ++i1)
        for (int64_t i2 = 0; i2 < c.n[2]; ++i2) {
          uint8_t* base = sb + i0 * c.st[0] + i1 * c.st[1] + i2 * c.st[2];
          for (int64_t r = 0; r < R; ++r) {
            const int64_t len = L ? L : pre[r + 1] - pre[r];
            uint8_t* sp = base + (offs ? offs[r] : 0);
            if (dir == 0) std::memcpy(pp, sp, size_t(len));
            else std::memcpy(sp, pp, size_t(len));
            pp += len;
          }
        }
    return;
  }
  TcArgs a;
  a.strided = reinterpret_cast<uint8_t*>(strided);
  a.packed = reinterpret_cast<uint8_t*>(packed);
  a.lay = make_layout(c, table, R, L, per, unit);
  a.dir = dir;
  const int mode = layout_mode(table, R, L);
  wide = wide || c.bytes >= (int64_t(1) << 32);
  const dim3 grid = layout_grid(a.lay.items, max_blocks);
  hip_check(hipSetDevice(dev), "hipSetDevice");
  switch (unit) {
    case 16: launch_unit<u32x4>(wide, mode, grid, s, a); break;
    case 8: launch_unit<u32x2>(wide, mode, grid, s, a); break;
    case 4: launch_unit<uint32_t>(wide, mode, grid, s, a); break;
    case 2: launch_unit<uint16_t>(wide, mode, grid, s, a); break;
    default: launch_unit<uint8_t>(wide, mode, grid, s, a); break;
  }
  hip_check(hipGetLastError(), "type_copy launch");
}

}  // namespace mpit
