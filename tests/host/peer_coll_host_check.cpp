// Stand-alone check of the host twins (dev = -1) of peer_gather, peer_fold and peer_scan for
// sanitizer builds: every buffer is a heap block of exactly the bytes the call may touch, so
// AddressSanitizer sees any access outside it, and every result is compared with a plain
// per-element loop. Cases: the segment lengths and misalignments of the kernel tests
// (peer_gather), counts {1, 3, 1031, 65541} x 1, 2, 3, 5 and 8 sources on int32 SUM, float SUM
// and uint8 BXOR (peer_fold), inclusive and exclusive, in place and out of place (peer_scan; the
// exclusive form gets no dst[0] at all). No GPU is used.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++20 -Icsrc -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tests/host/peer_coll_host_check.cpp \
//       csrc/kernels/peer_coll.hip csrc/kernels/allreduce.hip -o peer_coll_host_check && ./peer_coll_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "kernels/kernels.h"

namespace {

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int failures = 0;
void fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  ++failures;
}

// a heap block of exactly `bytes` bytes (at least one, so that it has an address) filled at random
uint8_t* block(int64_t bytes) {
  uint8_t* p = static_cast<uint8_t*>(std::malloc(size_t(bytes > 0 ? bytes : 1)));
  for (int64_t i = 0; i < bytes; ++i) p[i] = uint8_t(rnd());
  return p;
}

void check_gather() {
  const int64_t lens[8] = {0, 1, 15, 16, 17, 4099, 262164, 33};
  for (int ng : {8, 1})
    for (int rot = 0; rot < 8; ++rot) {
      std::vector<uint8_t*> src, dst;
      std::vector<uintptr_t> sp, dp;
      std::vector<int64_t> nb;
      for (int g = 0; g < ng; ++g) {
        const int64_t n = lens[(g + rot) % 8];
        src.push_back(block(n));
        dst.push_back(block(n));
        sp.push_back(reinterpret_cast<uintptr_t>(src.back()));
        dp.push_back(reinterpret_cast<uintptr_t>(dst.back()));
        nb.push_back(n);
      }
      mpit::peer_gather(-1, nullptr, sp, dp, nb, rot % 3);
      for (int g = 0; g < ng; ++g) {
        if (std::memcmp(src[size_t(g)], dst[size_t(g)], size_t(nb[size_t(g)])) != 0) fail("peer_gather", ng, rot, g);
        std::free(src[size_t(g)]);
        std::free(dst[size_t(g)]);
      }
    }
}

template <class T>
T comb(int op, T a, T b) {
  return op == mpit::kPrSum ? T(a + b) : T(a ^ b);
}
template <>
float comb<float>(int, float a, float b) {
  return a + b;
}
template <>
int32_t comb<int32_t>(int op, int32_t a, int32_t b) {
  return op == mpit::kPrSum ? int32_t(uint32_t(a) + uint32_t(b)) : (a ^ b);
}

template <class T>
void fill(T* p, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t r = rnd();
    if constexpr (std::is_same_v<T, float>) p[i] = float(int32_t(r & 0xffff) - 32768) * (1.0f / float(1 + (r >> 16) % 97));
    else p[i] = T(r);
  }
}

template <class T>
void check_fold_scan(int dtype, int op) {
  for (int64_t n : {1, 3, 1031, 65541})
    for (int ns : {1, 2, 3, 5, 8}) {
      std::vector<T*> src;
      std::vector<uintptr_t> sp;
      for (int k = 0; k < ns; ++k) {
        src.push_back(static_cast<T*>(std::malloc(size_t(n) * sizeof(T))));
        fill(src.back(), n);
        sp.push_back(reinterpret_cast<uintptr_t>(src.back()));
      }
      // prefix[j][i], a plain loop
      std::vector<std::vector<T>> pre(static_cast<size_t>(ns), std::vector<T>(size_t(n)));
      for (int64_t i = 0; i < n; ++i) {
        T acc = src[0][i];
        pre[0][size_t(i)] = acc;
        for (int k = 1; k < ns; ++k) pre[size_t(k)][size_t(i)] = acc = comb<T>(op, acc, src[size_t(k)][i]);
      }
      T* out = static_cast<T*>(std::malloc(size_t(n) * sizeof(T)));
      mpit::peer_fold(-1, nullptr, op, dtype, sp, reinterpret_cast<uintptr_t>(out), n, ns % 2);
      if (std::memcmp(out, pre[size_t(ns - 1)].data(), size_t(n) * sizeof(T)) != 0) fail("peer_fold", dtype, n, ns);
      std::free(out);
      for (int excl = 0; excl < 2; ++excl) {
        // out of place: one exact block per destination, none for dst[0] of the exclusive form
        std::vector<T*> dst(static_cast<size_t>(ns), nullptr);
        std::vector<uintptr_t> dp(static_cast<size_t>(ns), 0);
        for (int j = excl; j < ns; ++j) {
          dst[size_t(j)] = static_cast<T*>(std::malloc(size_t(n) * sizeof(T)));
          dp[size_t(j)] = reinterpret_cast<uintptr_t>(dst[size_t(j)]);
        }
        mpit::peer_scan(-1, nullptr, op, dtype, excl != 0, sp, dp, n, 0);
        for (int j = excl; j < ns; ++j) {
          if (std::memcmp(dst[size_t(j)], pre[size_t(j - excl)].data(), size_t(n) * sizeof(T)) != 0)
            fail("peer_scan", dtype, n, ns * 10 + excl);
          std::free(dst[size_t(j)]);
        }
        // in place on copies of the sources
        std::vector<T*> work;
        std::vector<uintptr_t> wp;
        for (int k = 0; k < ns; ++k) {
          work.push_back(static_cast<T*>(std::malloc(size_t(n) * sizeof(T))));
          std::memcpy(work.back(), src[size_t(k)], size_t(n) * sizeof(T));
          wp.push_back(reinterpret_cast<uintptr_t>(work.back()));
        }
        mpit::peer_scan(-1, nullptr, op, dtype, excl != 0, wp, wp, n, 0);
        for (int j = 0; j < ns; ++j) {
          const T* want = (excl && j == 0) ? src[0] : pre[size_t(j - excl)].data();
          if (std::memcmp(work[size_t(j)], want, size_t(n) * sizeof(T)) != 0)
            fail("peer_scan in place", dtype, n, ns * 10 + excl);
          std::free(work[size_t(j)]);
        }
      }
      for (T* p : src) std::free(p);
    }
}

}  // namespace

int main() {
  check_gather();
  check_fold_scan<int32_t>(mpit::kPrI32, mpit::kPrSum);
  check_fold_scan<float>(mpit::kPrF32, mpit::kPrSum);
  check_fold_scan<uint8_t>(mpit::kPrU8, mpit::kPrBxor);
  if (failures) {
    std::printf("%d FAILURES\n", failures);
    return 1;
  }
  std::printf("peer_coll host twins: OK\n");
  return 0;
}
