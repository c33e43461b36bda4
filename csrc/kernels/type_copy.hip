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

namespace mpit {
namespace {

constexpr int kTB = 256;
constexpr int kPerThread = 4;
constexpr int64_t kTile = int64_t(kTB) * kPerThread;
constexpr int kLdsRuns = 1024;
constexpr int kMaxBlocks = 2048;

// plain clang vectors: an array of them stays in registers (HIP's uint4 wrapper class went to scratch)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct TcArgs {
  uint8_t* strided;
  uint8_t* packed;
  const int64_t* table;
  int64_t n1, n2;  // the two inner loop counts (the outermost is implied by `items`)
  int64_t s0, s1, s2;
  int64_t R, L, per;  // per = packed bytes of one innermost iteration
  int64_t items;
  int dir;  // 0 gather strided -> packed, 1 scatter packed -> strided
  int lds;
};

// MODE 0: one run at offset 0; 1: equal-length runs; 2: prefix-sum search
template <typename V, typename IT, int MODE>
__global__ __launch_bounds__(kTB) void type_copy_kernel(TcArgs a) {
  __shared__ int64_t sh[MODE == 0 ? 1 : 2 * kLdsRuns + 1];
  const int64_t* offs = a.table;
  const int64_t* pre = a.table + a.R;
  if (MODE != 0 && a.lds) {
    const int nw = int(MODE == 1 ? a.R : 2 * a.R + 1);
    for (int i = threadIdx.x; i < nw; i += kTB) sh[i] = a.table[i];
    __syncthreads();
    offs = sh;
    pre = sh + a.R;
  }
  const IT per = IT(a.per), L = IT(a.L), n1 = IT(a.n1), n2 = IT(a.n2);
  const int64_t step = int64_t(gridDim.x) * kTile;
  for (int64_t t0 = int64_t(blockIdx.x) * kTile; t0 < a.items; t0 += step) {
    V v[kPerThread];
    uint8_t* dst[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const int64_t i = t0 + j * kTB + threadIdx.x;
      dst[j] = nullptr;
      if (i < a.items) {
        const IT q = IT(i) * IT(sizeof(V));
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
        uint8_t* sp = a.strided + off + int64_t(rem);
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
  if (loops.size() > 3) bad("at most three loops");
  if (unit != 1 && unit != 2 && unit != 4 && unit != 8 && unit != 16) bad("unit is a power of two <= 16");
  if (R < 1 || L < 0 || per <= 0) bad("R >= 1, L >= 0 and per > 0");
  if (L != 0 && per != R * L) bad("per != R * L");
  if (!table && !(R == 1 && L != 0)) bad("a run table is needed unless R == 1 with L != 0");
  if (per % unit || L % unit || strided % uintptr_t(unit) || packed % uintptr_t(unit)) bad("unit does not divide the layout");
  int64_t n[3] = {1, 1, 1}, st[3] = {0, 0, 0};
  unsigned __int128 total = uint64_t(per);
  for (size_t k = 0; k < loops.size(); ++k) {
    const size_t at = 3 - loops.size() + k;
    n[at] = loops[k][0];
    st[at] = loops[k][1];
    if (n[at] < 0) bad("negative loop count");
    if (n[at] > 1 && st[at] % unit) bad("unit does not divide a loop stride");
    total *= uint64_t(n[at]);
    if (total >> 62) bad("packed size overflows");
  }
  if (total == 0) return;
  const int64_t bytes = int64_t(total);
  if (dev < 0) {
    const int64_t* offs = reinterpret_cast<const int64_t*>(table);
    const int64_t* pre = offs ? offs + R : nullptr;
    uint8_t* sb = reinterpret_cast<uint8_t*>(strided);
    uint8_t* pp = reinterpret_cast<uint8_t*>(packed);
    for (int64_t i0 = 0; i0 < n[0]; ++i0)
      for (int64_t i1 = 0; i1 < n[1]; ++i1)
        for (int64_t i2 = 0; i2 < n[2]; ++i2) {
          uint8_t* base = sb + i0 * st[0] + i1 * st[1] + i2 * st[2];
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
  a.table = reinterpret_cast<const int64_t*>(table);
  a.n1 = n[1];
  a.n2 = n[2];
  a.s0 = st[0];
  a.s1 = st[1];
  a.s2 = st[2];
  a.R = R;
  a.L = L;
  a.per = per;
  a.items = bytes / unit;
  a.dir = dir;
  a.lds = R <= kLdsRuns;
  const int mode = L == 0 ? 2 : (R == 1 && !table ? 0 : 1);
  wide = wide || bytes >= (int64_t(1) << 32);
  int64_t cap = kMaxBlocks;
  if (max_blocks > 0) cap = std::min<int64_t>(cap, max_blocks);
  const dim3 grid(unsigned(std::min<int64_t>((a.items + kTile - 1) / kTile, cap)));
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
