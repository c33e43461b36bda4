// Stand-alone check of type_accumulate's host twin (dev = -1) for sanitizer builds: every buffer
// is a heap block of exactly the bytes the layout may touch, so AddressSanitizer sees any access
// outside it, and the result is compared with a plain per-element loop. Cases: the three run
// modes (one run without a table; 2, 3, 65, 1,024 and 1,025 runs of equal and of unequal
// lengths) under a count loop, and the tile seams (1,023 .. 2,049 items). No GPU is used.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++20 -Icsrc -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tests/host/type_acc_host_check.cpp \
//       csrc/kernels/type_acc.hip csrc/kernels/allreduce.hip -o type_acc_host_check && ./type_acc_host_check
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels/kernels.h"

namespace {

uint32_t rng_state = 12345;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int failures = 0;

// R runs (element counts lens[r] at element offsets offs[r]) repeated `count` times every `extent` elements
void run_case(const char* name, const std::vector<int64_t>& offs, const std::vector<int64_t>& lens, int64_t count,
              int64_t extent, int op, bool fetch, bool use_table) {
  const int64_t R = int64_t(lens.size());
  std::vector<int64_t> table(size_t(2 * R + 1));
  int64_t per = 0, hi = 0;
  bool equal = true;
  for (int64_t r = 0; r < R; ++r) {
    table[size_t(r)] = offs[size_t(r)] * 4;
    table[size_t(R + r)] = per * 4;
    per += lens[size_t(r)];
    hi = std::max(hi, offs[size_t(r)] + lens[size_t(r)]);
    equal = equal && lens[size_t(r)] == lens[0];
  }
  table[size_t(2 * R)] = per * 4;
  const int64_t span = (count - 1) * extent + hi, n = per * count;
  int32_t* target = static_cast<int32_t*>(std::malloc(size_t(span) * 4));
  int32_t* origin = static_cast<int32_t*>(std::malloc(size_t(n) * 4));
  int32_t* fetched = static_cast<int32_t*>(std::malloc(size_t(n) * 4));
  const size_t nspan = size_t(span);
  std::vector<int32_t> want(nspan), want_f(size_t(n), -7), old(nspan);
  for (int64_t i = 0; i < span; ++i) target[i] = old[size_t(i)] = want[size_t(i)] = int32_t(rnd());
  for (int64_t i = 0; i < n; ++i) {
    origin[i] = int32_t(rnd());
    fetched[i] = -7;
  }
  int64_t q = 0;
  for (int64_t c = 0; c < count; ++c)
    for (int64_t r = 0; r < R; ++r)
      for (int64_t e = 0; e < lens[size_t(r)]; ++e, ++q) {
        const int64_t at = c * extent + offs[size_t(r)] + e;
        const uint32_t a = uint32_t(old[size_t(at)]), b = uint32_t(origin[q]);
        want[size_t(at)] = op == mpit::kPrSum ? int32_t(a + b) : (op == mpit::kAccReplace ? int32_t(b) : int32_t(a ^ b));
        if (fetch) want_f[size_t(q)] = int32_t(a);
      }
  std::vector<std::array<int64_t, 2>> loops;
  if (count > 1) loops.push_back({count, extent * 4});
  mpit::type_accumulate(-1, nullptr, op, mpit::kPrI32, reinterpret_cast<uintptr_t>(target),
                        reinterpret_cast<uintptr_t>(origin), fetch ? reinterpret_cast<uintptr_t>(fetched) : 0, loops,
                        use_table ? reinterpret_cast<uintptr_t>(table.data()) : 0, R, equal ? lens[0] * 4 : 0, per * 4, 4);
  const bool ok = !std::memcmp(target, want.data(), size_t(span) * 4) && !std::memcmp(fetched, want_f.data(), size_t(n) * 4);
  std::printf("%s %s R=%lld count=%lld\n", ok ? "ok  " : "FAIL", name, static_cast<long long>(R), static_cast<long long>(count));
  failures += !ok;
  std::free(target);
  std::free(origin);
  std::free(fetched);
}

}  // namespace

int main() {
  run_case("one run, no table", {0}, {37}, 3, 50, mpit::kPrSum, true, false);
  for (int64_t R : {2, 3, 65, 1024, 1025})
    for (int equal = 0; equal < 2; ++equal) {
      std::vector<int64_t> offs, lens;
      int64_t at = 0;
      for (int64_t r = 0; r < R; ++r) {
        const int64_t len = equal ? 2 : 1 + int64_t(rnd() % 16);
        offs.push_back(at);
        lens.push_back(len);
        at += len + 1 + int64_t(rnd() % 8);
      }
      run_case(equal ? "equal runs" : "unequal runs", offs, lens, 2, at + 3, equal ? mpit::kPrBxor : mpit::kPrSum, !equal, true);
    }
  for (int64_t items : {1023, 1024, 1025, 2047, 2048, 2049})
    run_case("tile seam", {0}, {1}, items, 3, mpit::kAccReplace, true, false);
  if (failures) std::printf("%d case(s) failed\n", failures);
  return failures ? 1 : 0;
}
