// The element types and the combine of the predefined reductions, shared by the window
// all-reduce (allreduce.hip) and the one-sided accumulate (type_acc.hip) so that both give the
// same bits for the same operands: bf16 / fp16 widen to fp32 and round once, integers wrap,
// MAX / MIN propagate NaN, LAND / LOR / LXOR give 0 or 1 in the dtype, the bitwise ops are
// integer-only (peer_reduce_supported). Host and device run the same functions.
#pragma once
#include <cstdint>
#include <type_traits>

#include "ew.h"
#include "kernels.h"

// plain IEEE operations in the stated order: no contraction in this header nor, from here on,
// in the file that includes it
#pragma clang fp contract(off)

namespace mpit {

// element tags: S storage type, A accumulator type
struct TF32 { using S = float; using A = float; static constexpr bool kInt = false; };
struct TBf16 { using S = uint16_t; using A = float; static constexpr bool kInt = false; };
struct TF16 { using S = uint16_t; using A = float; static constexpr bool kInt = false; };
struct TF64 { using S = double; using A = double; static constexpr bool kInt = false; };
struct TI32 { using S = int32_t; using A = int32_t; using U = uint32_t; static constexpr bool kInt = true; };
struct TI64 { using S = int64_t; using A = int64_t; using U = uint64_t; static constexpr bool kInt = true; };
struct TU8 { using S = uint8_t; using A = uint8_t; using U = uint8_t; static constexpr bool kInt = true; };

template <class Tag>
MPIT_HD typename Tag::A widen(typename Tag::S v) {
  if constexpr (std::is_same_v<Tag, TBf16>) return bf2f(v);
  else if constexpr (std::is_same_v<Tag, TF16>) return float(__builtin_bit_cast(_Float16, v));
  else return v;
}
template <class Tag>
MPIT_HD typename Tag::S narrow(typename Tag::A v) {
  if constexpr (std::is_same_v<Tag, TBf16>) return f2bf(v);
  else if constexpr (std::is_same_v<Tag, TF16>) return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
  else return v;
}

template <class Tag, int OP>
MPIT_HD typename Tag::A comb(typename Tag::A a, typename Tag::A b) {
  using A = typename Tag::A;
  if constexpr (OP == kPrLand) return A((a != A(0)) && (b != A(0)) ? 1 : 0);
  else if constexpr (OP == kPrLor) return A((a != A(0)) || (b != A(0)) ? 1 : 0);
  else if constexpr (OP == kPrLxor) return A((a != A(0)) != (b != A(0)) ? 1 : 0);
  else if constexpr (Tag::kInt) {
    using U = typename Tag::U;  // wrap-around like torch, without signed overflow
    if constexpr (OP == kPrSum) return A(U(U(a) + U(b)));
    else if constexpr (OP == kPrProd) return A(U(U(a) * U(b)));
    else if constexpr (OP == kPrMax) return a > b ? a : b;
    else if constexpr (OP == kPrMin) return a < b ? a : b;
    else if constexpr (OP == kPrBand) return A(a & b);
    else if constexpr (OP == kPrBor) return A(a | b);
    else return A(a ^ b);
  } else {
    if constexpr (OP == kPrSum) return a + b;
    else if constexpr (OP == kPrProd) return a * b;
    else if constexpr (OP == kPrMax) return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));  // NaN propagates
    else if constexpr (OP == kPrMin) return (a != a) ? a : ((b != b) ? b : (a < b ? a : b));
    else return a;  // bitwise ops on floats: peer_reduce_supported says no
  }
}

// the pointer table of the peer kernels (allreduce.hip, peer_coll.hip): by value in the kernel arguments
struct PeerTable {
  uint64_t src[kPeerMax];
  uint64_t dst[kPeerMax];
  int32_t ns, nd;
};

// x[0][e] = x[0][e] op x[1][e] op ... op x[ns-1][e]
template <class Tag, int OP, int NS, int VE>
MPIT_HD void fold(typename Tag::A (&x)[NS][VE], int ns) {
#pragma unroll
  for (int k = 1; k < NS; ++k) {
    if (k < ns) {
#pragma unroll
      for (int e = 0; e < VE; ++e) x[0][e] = comb<Tag, OP>(x[0][e], x[k][e]);
    }
  }
}

template <class Tag, int NS, int VE>
MPIT_HD void fold_op(int op, typename Tag::A (&x)[NS][VE], int ns) {
  switch (op) {
    case kPrSum: fold<Tag, kPrSum, NS, VE>(x, ns); break;
    case kPrProd: fold<Tag, kPrProd, NS, VE>(x, ns); break;
    case kPrMax: fold<Tag, kPrMax, NS, VE>(x, ns); break;
    case kPrMin: fold<Tag, kPrMin, NS, VE>(x, ns); break;
    case kPrLand: fold<Tag, kPrLand, NS, VE>(x, ns); break;
    case kPrLor: fold<Tag, kPrLor, NS, VE>(x, ns); break;
    case kPrLxor: fold<Tag, kPrLxor, NS, VE>(x, ns); break;
    default:
      if constexpr (Tag::kInt) {
        if (op == kPrBand) fold<Tag, kPrBand, NS, VE>(x, ns);
        else if (op == kPrBor) fold<Tag, kPrBor, NS, VE>(x, ns);
        else fold<Tag, kPrBxor, NS, VE>(x, ns);
      }
      break;
  }
}

}  // namespace mpit
