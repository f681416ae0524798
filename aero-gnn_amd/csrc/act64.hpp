// MLP hidden activations in float64 (AGN_ACT_*; torch's formulas, as common.hpp act_fwd / act_bwd),
// shared by the float64 GEMM epilogues (f64.hip) and the float64 activation + dropout (dropout.hip).
#pragma once
#include "common.hpp"

namespace agn {

AGN_DEV double act_fwd64(int k, double x) {
  if (k == AGN_ACT_GELU) return x * 0.5 * (1.0 + erf(x * 0.70710678118654752440));
  if (k == AGN_ACT_SILU) return x / (1.0 + exp(-x));
  if (k == AGN_ACT_TANH) return tanh(x);
  return x > 0.0 ? x : 0.0;
}
AGN_DEV double act_bwd64(int k, double x, double dy) {
  if (k == AGN_ACT_GELU) {
    const double cdf = 0.5 * (1.0 + erf(x * 0.70710678118654752440));
    const double pdf = exp(-0.5 * x * x) * 0.39894228040143267794;
    return dy * (cdf + x * pdf);
  }
  if (k == AGN_ACT_SILU) {
    const double sg = 1.0 / (1.0 + exp(-x));
    return dy * sg * (1.0 + x * (1.0 - sg));
  }
  if (k == AGN_ACT_TANH) {
    const double y = tanh(x);
    return dy * (1.0 - y * y);
  }
  return x > 0.0 ? dy : 0.0;
}

}  // namespace agn
