// The element types, the combine and the op switch (with_peer_op) of the predefined reductions,
// shared by the window all-reduce and fold (allreduce.hip), the window scan (peer_coll.hip) and
// the one-sided accumulate (type_acc.hip) so that all give the same bits for the same operands.
// The streaming frame of the first three is peer_stream.h, next to this header.
// bf16 / fp16 widen to fp32 and round once, integers wrap,
// MAX / MIN propagate NaN, LAND / LOR / LXOR give 0 or 1 in the dtype, the bitwise ops are
// integer-only (peer_reduce_supported). MAXLOC / MINLOC run on pair tags only: the element is a
// whole (value, index) pair and the combine selects one operand, copied unchanged.
// Host and device run the same functions.
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
struct TScalar { static constexpr bool kPair = false; };
struct TF32 : TScalar { using S = float; using A = float; static constexpr bool kInt = false; };
struct TBf16 : TScalar { using S = uint16_t; using A = float; static constexpr bool kInt = false; };
struct TF16 : TScalar { using S = uint16_t; using A = float; static constexpr bool kInt = false; };
struct TF64 : TScalar { using S = double; using A = double; static constexpr bool kInt = false; };
struct TI32 : TScalar { using S = int32_t; using A = int32_t; using U = uint32_t; static constexpr bool kInt = true; };
struct TI64 : TScalar { using S = int64_t; using A = int64_t; using U = uint64_t; static constexpr bool kInt = true; };
struct TU8 : TScalar { using S = uint8_t; using A = uint8_t; using U = uint8_t; static constexpr bool kInt = true; };

// A (value, index) pair of MAXLOC / MINLOC: value tag VT at byte 0, index tag IT at byte IOFF,
// EXT bytes in all (padding included). The storage is the whole pair, aligned like its largest
// member only: a float32 pair may sit at 4 mod 8. widen / narrow are the identity, so the pair
// that wins keeps every byte: the sign of zero, a NaN's payload, padding, 16-bit values.
template <class VT, class IT, int IOFF, int EXT>
struct TPair {
  using VTag = VT;
  using ITag = IT;
  static constexpr int kIdxOff = IOFF;
  static constexpr int kAlign = int(sizeof(typename VT::S) > sizeof(typename IT::S) ? sizeof(typename VT::S)
                                                                                    : sizeof(typename IT::S));
  struct alignas(kAlign) S { uint8_t b[EXT]; };
  using A = S;
  static constexpr bool kInt = false;
  static constexpr bool kPair = true;
  static_assert(EXT == 2 || EXT == 4 || EXT == 8 || EXT == 16, "a pair divides a 16-byte vector");
  static_assert(IOFF >= int(sizeof(typename VT::S)) && IOFF + int(sizeof(typename IT::S)) <= EXT && EXT % kAlign == 0,
                "the members lie inside the pair");
};
template <class T>
using THomPair = TPair<T, T, int(sizeof(typename T::S)), 2 * int(sizeof(typename T::S))>;  // interleaved, one dtype
using TFloatInt = TPair<TF32, TI32, 4, 8>;    // MPI_FLOAT_INT
using TDoubleInt = TPair<TF64, TI32, 8, 16>;  // MPI_DOUBLE_INT: 4 padding bytes
using TLongInt = TPair<TI64, TI32, 8, 16>;    // MPI_LONG_INT: 4 padding bytes

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

// true: MAXLOC / MINLOC (a, b) is b. The one definition of the rule (docs/ARCHITECTURE.md):
// both values NaN: the smaller index, a on equal or NaN indices; one value NaN: that pair;
// otherwise the better value, on equal values (-0 == +0) the smaller index, a on equal or NaN indices.
template <class Tag, bool MAX>
MPIT_HD bool loc_takes_b(const typename Tag::S& a, const typename Tag::S& b) {
  using VT = typename Tag::VTag;
  using IT = typename Tag::ITag;
  typename VT::S sva, svb;
  typename IT::S sia, sib;
  __builtin_memcpy(&sva, a.b, sizeof(sva));
  __builtin_memcpy(&svb, b.b, sizeof(svb));
  __builtin_memcpy(&sia, a.b + Tag::kIdxOff, sizeof(sia));
  __builtin_memcpy(&sib, b.b + Tag::kIdxOff, sizeof(sib));
  const typename VT::A va = widen<VT>(sva), vb = widen<VT>(svb);  // 16-bit floats compare exactly in fp32
  const typename IT::A ia = widen<IT>(sia), ib = widen<IT>(sib);
  const bool an = va != va, bn = vb != vb;
  if (an != bn) return bn;
  if (!an) {
    if (MAX ? vb > va : vb < va) return true;
    if (MAX ? va > vb : va < vb) return false;
  }
  return ib < ia;  // false when either index is NaN
}

template <class Tag, int OP>
MPIT_HD typename Tag::A comb(typename Tag::A a, typename Tag::A b) {
  using A = typename Tag::A;
  if constexpr (Tag::kPair) return loc_takes_b<Tag, OP == kPrMaxloc>(a, b) ? b : a;
  else if constexpr (OP == kPrLand) return A((a != A(0)) && (b != A(0)) ? 1 : 0);
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

// The one switch over the ten PeerOp: f(std::integral_constant<int, OP>{}) is called once for an
// (op, Tag) that peer_reduce_supported allows. A pair tag has the two pair ops and nothing else,
// a scalar tag the seven common ops, an integer tag the three bitwise ops as well. `op` is
// wave-uniform: callers switch once per vector / item, outside their element loops.
template <class Tag, class F>
MPIT_HD void with_peer_op(int op, F&& f) {
  if constexpr (Tag::kPair) {
    if (op == kPrMaxloc) f(std::integral_constant<int, kPrMaxloc>{});
    else f(std::integral_constant<int, kPrMinloc>{});
  } else {
    switch (op) {
      case kPrSum: f(std::integral_constant<int, kPrSum>{}); break;
      case kPrProd: f(std::integral_constant<int, kPrProd>{}); break;
      case kPrMax: f(std::integral_constant<int, kPrMax>{}); break;
      case kPrMin: f(std::integral_constant<int, kPrMin>{}); break;
      case kPrLand: f(std::integral_constant<int, kPrLand>{}); break;
      case kPrLor: f(std::integral_constant<int, kPrLor>{}); break;
      case kPrLxor: f(std::integral_constant<int, kPrLxor>{}); break;
      default:
        if constexpr (Tag::kInt) {
          if (op == kPrBand) f(std::integral_constant<int, kPrBand>{});
          else if (op == kPrBor) f(std::integral_constant<int, kPrBor>{});
          else f(std::integral_constant<int, kPrBxor>{});
        }
        break;
    }
  }
}

template <class Tag, int NS, int VE>
MPIT_HD void fold_op(int op, typename Tag::A (&x)[NS][VE], int ns) {
  with_peer_op<Tag>(op, [&](auto o) { fold<Tag, decltype(o)::value>(x, ns); });
}

// one call per element type of a PeerDtype code the caller has checked (peer_reduce_supported)
template <class F>
void with_peer_tag(int dtype, F&& f) {
  switch (dtype) {
    case kPrF32: f(TF32{}); break;
    case kPrBf16: f(TBf16{}); break;
    case kPrF16: f(TF16{}); break;
    case kPrF64: f(TF64{}); break;
    case kPrI32: f(TI32{}); break;
    case kPrI64: f(TI64{}); break;
    case kPrU8: f(TU8{}); break;
    case kPrPair + kPrF32: f(THomPair<TF32>{}); break;
    case kPrPair + kPrBf16: f(THomPair<TBf16>{}); break;
    case kPrPair + kPrF16: f(THomPair<TF16>{}); break;
    case kPrPair + kPrF64: f(THomPair<TF64>{}); break;
    case kPrPair + kPrI32: f(THomPair<TI32>{}); break;
    case kPrPair + kPrI64: f(THomPair<TI64>{}); break;
    case kPrPair + kPrU8: f(THomPair<TU8>{}); break;
    case kPrFloatInt: f(TFloatInt{}); break;
    case kPrDoubleInt: f(TDoubleInt{}); break;
    default: f(TLongInt{}); break;
  }
}

}  // namespace mpit
