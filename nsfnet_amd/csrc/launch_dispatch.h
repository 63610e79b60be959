// How the sweep and dW launchers turn run-time values into template arguments: the padded width, the mode (streams
// and bf16 terms) and the variant of the point stage.  Host-only C++17 without a HIP include, so it compiles
// stand-alone (tests/test_launch_dispatch_cpu.py).  Every launch_* is dispatch_width -> dispatch_ns_terms ->
// dispatch_variant -> its file's launch_one<...>; capi.hip's FAMILY_VARIANTS holds the same masks per family.
#pragma once
#include <type_traits>

// What a launcher returns for a width, mode or variant it has no kernel for (capi.hip reports it as -22).
constexpr int DISPATCH_UNSUPPORTED = -1000;

// f(std::integral_constant<int, W>{}) for the W that equals HP, `other` where none does.
template <int... W, class R, class F>
static R dispatch_width(int HP, R other, F f) {
  R r = other;
  (void)((HP == W && ((void)(r = f(std::integral_constant<int, W>{})), true)) || ...);
  return r;
}

// A sweep's run-time mode as template arguments: f(ns, terms) with NS = 4 (residual) / 1 (value) streams and TERMS = 3
// (bf16x3) / 1 (bf16) products per term, each a std::integral_constant.
template <class F>
static int dispatch_ns_terms(int NS, int terms, F f) {
  using std::integral_constant;
  if (terms == 3) return NS == 4 ? f(integral_constant<int, 4>{}, integral_constant<int, 3>{}) : f(integral_constant<int, 1>{}, integral_constant<int, 3>{});
  return NS == 4 ? f(integral_constant<int, 4>{}, integral_constant<int, 1>{}) : f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
}

// The variants of a sweep, one bit each: the plain tanh net, hard walls, the pseudo-time term, both, and the frozen
// sine first layer (which comes with neither).
enum : unsigned { VAR_TANH = 1, VAR_HBC = 2, VAR_PT = 4, VAR_HBC_PT = 8, VAR_FF = 16 };
constexpr unsigned variant_bit(bool hbc, bool ptime, bool ff) {
  return ff ? (hbc || ptime ? 0u : VAR_FF) : ptime ? (hbc ? VAR_HBC_PT : VAR_PT) : hbc ? VAR_HBC : VAR_TANH;
}
template <bool HBC, bool PT, bool FF>
struct Variant {
  static constexpr bool hbc = HBC, pt = PT, ff = FF;
  static constexpr unsigned bit = variant_bit(HBC, PT, FF);
};

// The variants each kind of launcher has kernels for.  FAMILY_VARIANTS (capi.hip) is built from the same names.
constexpr unsigned VARIANTS_ALL = VAR_TANH | VAR_HBC | VAR_PT | VAR_HBC_PT | VAR_FF;
constexpr unsigned VARIANTS_WAVE8 = VARIANTS_ALL;                               // 8-wave families, residual mode
constexpr unsigned VARIANTS_WAVE8_FWD_VALUE = VAR_TANH | VAR_HBC | VAR_FF;      // their forward in value mode
constexpr unsigned VARIANTS_WAVE8_BWD = VARIANTS_ALL & ~VAR_FF;                 // their reverse sweep: the plain kernel serves a sine net
constexpr unsigned VARIANTS_WAVE8_BWD_VALUE = VAR_TANH;                         // value mode takes adjoints that carry everything
constexpr unsigned VARIANTS_SPLIT = VARIANTS_ALL;                               // role-split, wide role-split, fused
constexpr unsigned VARIANTS_PIPE = VAR_TANH;                                    // pipelined schedule

// f(Variant<...>{}) for the one variant the three flags name.  DISPATCH_UNSUPPORTED for ff with walls or pseudo-time
// and for a variant outside MASK, which is not instantiated either.
template <unsigned MASK, class V, class F>
static int call_variant(F& f) {
  if constexpr ((MASK & V::bit) != 0) return f(V{});
  else return DISPATCH_UNSUPPORTED;
}
template <unsigned MASK, class F>
static int dispatch_variant(bool hbc, bool ptime, bool ff, F f) {
  if (ff) return hbc || ptime ? DISPATCH_UNSUPPORTED : call_variant<MASK, Variant<false, false, true>>(f);
  if (ptime) return hbc ? call_variant<MASK, Variant<true, true, false>>(f) : call_variant<MASK, Variant<false, true, false>>(f);
  return hbc ? call_variant<MASK, Variant<true, false, false>>(f) : call_variant<MASK, Variant<false, false, false>>(f);
}
