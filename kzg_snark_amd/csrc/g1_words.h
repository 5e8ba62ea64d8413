// g1_words.h -- a G1 point <-> its canonical affine words: x | y, F::NW little-endian 32-bit words each (the point
// format of the C ABI), all zeros and a flag for infinity.  The ONE statement of both directions, shared by the
// kernels, the host finishing code and tests/shim/g1_bytes_shim.cpp (which compiles this text with g++): like ec.h,
// nothing here is device-only.
#pragma once
#include "ec.h"

namespace kzg {

// canonical words < p, from the top word down
template <class F>
static KZG_HD bool words_below_p(const uint32_t* w) {
  bool lt = false, gt = false;
#pragma unroll
  for (int k = F::NW - 1; k >= 0; --k) {
    const uint32_t pw = F::PW[k];
    if (!lt && !gt) { lt = w[k] < pw; gt = w[k] > pw; }
  }
  return lt;
}

// THE rule "canonical affine words -> a point": both coordinates below p and the point on the curve.
// x, y: the coordinates in Montgomery form, reduced (also when the rule fails)
template <class C>
static KZG_HD bool import_affine(const uint32_t* wx, const uint32_t* wy, Fe<typename C::Fp>& x, Fe<typename C::Fp>& y) {
  using F = typename C::Fp;
  using Fd = Field<F>;
  const bool below = words_below_p<F>(wx) && words_below_p<F>(wy);
  x = Fd::reduce(Fd::to_mont(Fd::from_words(wx)));
  y = Fd::reduce(Fd::to_mont(Fd::from_words(wy)));
  return below && Ec<C>::on_curve(x, y);
}

// the conversion alone, nothing checked: w = x | y (words >= p are taken modulo p); zeros and the flag for infinity
template <class C>
static KZG_HD Affine<C> affine_from_words(const uint32_t* w, bool inf) {
  using Fd = Field<typename C::Fp>;
  Affine<C> a;
  a.inf = inf;
  a.x = Fd::zero();
  a.y = Fd::zero();
  if (!inf) {
    a.x = Fd::reduce(Fd::to_mont(Fd::from_words(w)));
    a.y = Fd::reduce(Fd::to_mont(Fd::from_words(w + C::Fp::NW)));
  }
  return a;
}

// the reverse: w = x | y, all zeros for infinity; returns the infinity flag
template <class C>
static KZG_HD bool affine_to_words(const Affine<C>& a, uint32_t* w) {
  using Fd = Field<typename C::Fp>;
  constexpr int NW = C::Fp::NW;
  if (a.inf) {
#pragma unroll
    for (int k = 0; k < 2 * NW; ++k) w[k] = 0;
  } else {
    Fd::to_words(Fd::from_mont(a.x), w);
    Fd::to_words(Fd::from_mont(a.y), w + NW);
  }
  return a.inf;
}

}  // namespace kzg
