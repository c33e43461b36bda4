// Stand-alone check of the host twins (dev = -1) of the MAXLOC / MINLOC pair types in peer_reduce,
// peer_fold, peer_scan and type_accumulate, for sanitizer builds. Every buffer is a heap block
// that ends exactly where the call may touch last, so AddressSanitizer sees any access past it;
// a block at `mis` bytes past the allocator's 16-byte boundary starts `mis` bytes into its
// allocation (those bytes in front are the one slack there is; with mis = 0 there is none).
// Results are compared with a plain per-pair loop over typed members. Cases: float32 pairs and
// FLOAT_INT at 0 and at 4 mod 8 (aligned to the member, not to the pair: UBSan checks every typed
// access), DOUBLE_INT and LONG_INT (16 bytes, 4 of them padding that must travel with the pair)
// at 0 and at 8 mod 16; counts {1, 2, 3, 1031} x 1, 2, 3, 5 and 8 sources, every source at its
// own misalignment; inclusive and exclusive scans, in place and out of place (the exclusive form
// gets no dst[0] at all); type_accumulate on a contiguous target with and without a fetch stream,
// and its refusal of a unit smaller than the pair. No GPU is used.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++20 -Icsrc -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tests/host/pair_host_check.cpp \
//       csrc/kernels/peer_coll.hip csrc/kernels/allreduce.hip csrc/kernels/type_acc.hip \
//       -o pair_host_check && ./pair_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
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

// `bytes` bytes that start `mis` bytes into a heap block and end with it
struct Block {
  uint8_t* base;
  uint8_t* p;
  Block(int64_t bytes, int mis) : base(static_cast<uint8_t*>(std::malloc(size_t(bytes + mis)))), p(base + mis) {
    if (reinterpret_cast<uintptr_t>(base) % 16) std::abort();  // the allocator's alignment is assumed
    for (int64_t i = 0; i < bytes; ++i) p[i] = uint8_t(rnd());
  }
  Block(const Block&) = delete;
  ~Block() { std::free(base); }
  uintptr_t addr() const { return reinterpret_cast<uintptr_t>(p); }
};

template <class T>
T pick(bool index) {
  const uint32_t r = rnd();
  if (index) {
    if constexpr (std::is_floating_point_v<T>) return r % 29 == 0 ? T(NAN) : T(r % 6);
    else return T(r % 6);
  }
  if constexpr (std::is_floating_point_v<T>) {
    const T table[9] = {T(0.0), T(-0.0), T(1), T(2), T(-1), T(3), T(INFINITY), T(-INFINITY), T(NAN)};
    return table[r % 9];
  } else {
    return T(int(r % 6) - 2);
  }
}

// the rule in plain words, on typed members
template <class V, class I>
bool takes_b(const uint8_t* a, const uint8_t* b, int ioff, bool max) {
  V va, vb;
  I ia, ib;
  std::memcpy(&va, a, sizeof(V));
  std::memcpy(&vb, b, sizeof(V));
  std::memcpy(&ia, a + ioff, sizeof(I));
  std::memcpy(&ib, b + ioff, sizeof(I));
  const bool an = va != va, bn = vb != vb;
  if (an && bn) return ib < ia;
  if (an) return false;
  if (bn) return true;
  if (max ? vb > va : vb < va) return true;
  if (max ? va > vb : va < vb) return false;
  return ib < ia;
}

template <class V, class I>
void check_layout(int dtype, int ioff, int ext, int step) {
  // `step`: the member alignment; block k sits (k * step) % ext bytes off the pair's own alignment
  for (int op : {int(mpit::kPrMaxloc), int(mpit::kPrMinloc)})
    for (int64_t n : {1, 2, 3, 1031})
      for (int ns : {1, 2, 3, 5, 8}) {
        const int64_t nb = n * ext;
        std::vector<Block*> src;
        std::vector<uintptr_t> sp;
        for (int k = 0; k < ns; ++k) {
          src.push_back(new Block(nb, (k * step) % ext));  // random bytes: the padding differs everywhere
          for (int64_t i = 0; i < n; ++i) {
            const V v = pick<V>(false);
            const I x = pick<I>(true);
            std::memcpy(src.back()->p + i * ext, &v, sizeof(V));
            std::memcpy(src.back()->p + i * ext + ioff, &x, sizeof(I));
          }
          sp.push_back(src.back()->addr());
        }
        std::vector<std::vector<uint8_t>> pre(static_cast<size_t>(ns), std::vector<uint8_t>(size_t(nb)));
        for (int64_t i = 0; i < n; ++i) {
          const uint8_t* acc = src[0]->p + i * ext;
          std::memcpy(pre[0].data() + i * ext, acc, size_t(ext));
          for (int k = 1; k < ns; ++k) {
            const uint8_t* b = src[size_t(k)]->p + i * ext;
            if (takes_b<V, I>(acc, b, ioff, op == mpit::kPrMaxloc)) acc = b;
            std::memcpy(pre[size_t(k)].data() + i * ext, acc, size_t(ext));
          }
        }
        const uint8_t* all = pre[size_t(ns - 1)].data();
        {
          Block d0(nb, step % ext), d1(nb, 0);
          mpit::peer_reduce(-1, nullptr, op, dtype, sp, {d0.addr(), d1.addr()}, n);
          if (std::memcmp(d0.p, all, size_t(nb)) || std::memcmp(d1.p, all, size_t(nb))) fail("peer_reduce", dtype, n, ns);
          Block f(nb, step % ext);
          mpit::peer_fold(-1, nullptr, op, dtype, sp, f.addr(), n, ns % 2);
          if (std::memcmp(f.p, all, size_t(nb))) fail("peer_fold", dtype, n, ns);
        }
        for (int excl = 0; excl < 2; ++excl) {
          std::vector<Block*> dst(static_cast<size_t>(ns), nullptr);
          std::vector<uintptr_t> dp(static_cast<size_t>(ns), 0);
          for (int j = excl; j < ns; ++j) {
            dst[size_t(j)] = new Block(nb, ((j + 1) * step) % ext);
            dp[size_t(j)] = dst[size_t(j)]->addr();
          }
          mpit::peer_scan(-1, nullptr, op, dtype, excl != 0, sp, dp, n, 0);
          for (int j = excl; j < ns; ++j) {
            if (std::memcmp(dst[size_t(j)]->p, pre[size_t(j - excl)].data(), size_t(nb)))
              fail("peer_scan", dtype, n, ns * 10 + excl);
            delete dst[size_t(j)];
          }
          std::vector<Block*> work;
          std::vector<uintptr_t> wp;
          for (int k = 0; k < ns; ++k) {
            work.push_back(new Block(nb, (k * step) % ext));
            std::memcpy(work.back()->p, src[size_t(k)]->p, size_t(nb));
            wp.push_back(work.back()->addr());
          }
          mpit::peer_scan(-1, nullptr, op, dtype, excl != 0, wp, wp, n, 0);
          for (int j = 0; j < ns; ++j) {
            const uint8_t* want = (excl && j == 0) ? src[0]->p : pre[size_t(j - excl)].data();
            if (std::memcmp(work[size_t(j)]->p, want, size_t(nb))) fail("peer_scan in place", dtype, n, ns * 10 + excl);
            delete work[size_t(j)];
          }
        }
        if (ns >= 2) {  // target = source 0, origin = source 1: one contiguous run of n pairs, item = one pair
          for (int fetch = 0; fetch < 2; ++fetch) {
            Block t(nb, 0), o(nb, 0), f(nb, 0);
            std::memcpy(t.p, src[0]->p, size_t(nb));
            std::memcpy(o.p, src[1]->p, size_t(nb));
            std::vector<uint8_t> f0(f.p, f.p + nb);
            mpit::type_accumulate(-1, nullptr, op, dtype, t.addr(), o.addr(), fetch ? f.addr() : 0, {}, 0, 1, nb, nb, ext);
            if (std::memcmp(t.p, pre[1].data(), size_t(nb))) fail("type_accumulate", dtype, n, fetch);
            if (std::memcmp(o.p, src[1]->p, size_t(nb))) fail("type_accumulate origin", dtype, n, fetch);
            if (std::memcmp(f.p, fetch ? src[0]->p : f0.data(), size_t(nb))) fail("type_accumulate fetch", dtype, n, fetch);
          }
          Block t(nb, step % ext), o(nb, step % ext);  // aligned to the member only: the unit is below the pair
          std::vector<uint8_t> t0(t.p, t.p + nb);
          bool refused = false;
          try {
            mpit::type_accumulate(-1, nullptr, op, dtype, t.addr(), o.addr(), 0, {}, 0, 1, nb, nb, step);
          } catch (const std::invalid_argument&) {
            refused = true;
          }
          if (!refused || std::memcmp(t.p, t0.data(), size_t(nb))) fail("type_accumulate unit < pair", dtype, n, step);
        }
        for (Block* b : src) delete b;
      }
}

}  // namespace

int main() {
  check_layout<float, float>(mpit::kPrPair + mpit::kPrF32, 4, 8, 4);  // sources at 0 and at 4 mod 8
  check_layout<float, int32_t>(mpit::kPrFloatInt, 4, 8, 4);
  check_layout<double, int32_t>(mpit::kPrDoubleInt, 8, 16, 8);  // at 0 and at 8 mod 16
  check_layout<int64_t, int32_t>(mpit::kPrLongInt, 8, 16, 8);
  check_layout<int32_t, int32_t>(mpit::kPrPair + mpit::kPrI32, 4, 8, 4);  // 2INT
  if (failures) {
    std::printf("%d FAILURES\n", failures);
    return 1;
  }
  std::printf("pair host twins: OK\n");
  return 0;
}
