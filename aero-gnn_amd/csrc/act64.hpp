// MLP hidden activations in float64 (AGN_ACT_*; torch's formulas, as common.hpp act_fwd / act_bwd),
// shared by the float64 GEMM epilogues (f64.hip) and the float64 activation + dropout (dropout.hip).
#pragma once
#include "common.hpp"

namespace agn {

constexpr double SELU_SCALE64 = 1.0507009873554804934193349852946;
constexpr double SELU_NEG64 = 1.6732632423543772848170429916717 * 1.0507009873554804934193349852946;
// torch's hardsigmoid backward multiplies by the FLOAT 1/6 in every dtype (Activation.cpp
// `one_sixth(1.0f / 6.0f)`): 4.97e-9 above 1/6. Kept, so the float64 route agrees with the
// reference's own float64 gradients to its 1e-10 bar.
constexpr double ONE_SIXTH64 = (double)(1.0f / 6.0f);

AGN_DEV double sigmoid64(double x) {
  const double e = exp(-fabs(x));
  return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}
// x - tanh(x); the odd series below 1/32, where the difference cancels (next term < 2e-17 of the first)
AGN_DEV double tanhshrink64(double x) {
  if (fabs(x) >= 0.03125) return x - tanh(x);
  const double x2 = x * x;
  const double p = 1.0 / 3.0 + x2 * (-2.0 / 15.0 + x2 * (17.0 / 315.0 + x2 * (-62.0 / 2835.0 + x2 * (1382.0 / 155925.0))));
  return x * x2 * p;
}

AGN_DEV double act_fwd64(int k, double x) {
  switch (k) {
    case AGN_ACT_GELU: return x * 0.5 * (1.0 + erf(x * 0.70710678118654752440));
    case AGN_ACT_SILU: return x / (1.0 + exp(-x));
    case AGN_ACT_TANH: return tanh(x);
    case AGN_ACT_RELU6: return fmin(fmax(x, 0.0), 6.0);
    case AGN_ACT_HARDTANH: return fmin(fmax(x, -1.0), 1.0);
    case AGN_ACT_LEAKY_RELU: return x > 0.0 ? x : x * 0.01;
    case AGN_ACT_ELU:
    case AGN_ACT_CELU: return x > 0.0 ? x : expm1(x);
    case AGN_ACT_SELU: return x > 0.0 ? x * SELU_SCALE64 : expm1(x) * SELU_NEG64;
    case AGN_ACT_HARDSIGMOID: return fmin(fmax(x + 3.0, 0.0), 6.0) / 6.0;
    case AGN_ACT_HARDSWISH: return x * fmin(fmax(x + 3.0, 0.0), 6.0) / 6.0;
    case AGN_ACT_SOFTPLUS: return x > 20.0 ? x : log1p(exp(x));
    case AGN_ACT_SOFTSIGN: return x / (1.0 + fabs(x));
    case AGN_ACT_SIGMOID: return sigmoid64(x);
    case AGN_ACT_LOGSIGMOID: return fmin(x, 0.0) - log1p(exp(-fabs(x)));
    case AGN_ACT_MISH: return x * tanh(x > 20.0 ? x : log1p(exp(x)));
    case AGN_ACT_TANHSHRINK: return tanhshrink64(x);
    default: return x > 0.0 ? x : 0.0;
  }
}
AGN_DEV double act_bwd64(int k, double x, double dy) {
  switch (k) {
    case AGN_ACT_GELU: {
      const double cdf = 0.5 * (1.0 + erf(x * 0.70710678118654752440));
      const double pdf = exp(-0.5 * x * x) * 0.39894228040143267794;
      return dy * (cdf + x * pdf);
    }
    case AGN_ACT_SILU: {
      const double sg = 1.0 / (1.0 + exp(-x));
      return dy * sg * (1.0 + x * (1.0 - sg));
    }
    case AGN_ACT_TANH: {
      const double y = tanh(x);
      return dy * (1.0 - y * y);
    }
    case AGN_ACT_RELU6: return (x > 0.0 && x < 6.0) ? dy : 0.0;
    case AGN_ACT_HARDTANH: return (x > -1.0 && x < 1.0) ? dy : 0.0;
    case AGN_ACT_LEAKY_RELU: return x > 0.0 ? dy : dy * 0.01;
    case AGN_ACT_ELU:
    case AGN_ACT_CELU: return x > 0.0 ? dy : dy * exp(x);
    case AGN_ACT_SELU: return x > 0.0 ? dy * SELU_SCALE64 : dy * SELU_NEG64 * exp(x);
    case AGN_ACT_HARDSIGMOID: return (x > -3.0 && x < 3.0) ? dy * ONE_SIXTH64 : 0.0;
    case AGN_ACT_HARDSWISH: return x <= -3.0 ? 0.0 : (x < 3.0 ? dy * (x / 3.0 + 0.5) : dy);
    case AGN_ACT_SOFTPLUS: {
      if (x > 20.0) return dy;
      const double z = exp(x);
      return dy * z / (z + 1.0);
    }
    case AGN_ACT_SOFTSIGN: {
      const double d = 1.0 + fabs(x);
      return dy / (d * d);
    }
    case AGN_ACT_SIGMOID: {
      const double y = sigmoid64(x);
      return dy * (1.0 - y) * y;
    }
    case AGN_ACT_LOGSIGMOID: {
      const double z = exp(-fabs(x));
      const double q = z / (1.0 + z);
      return dy * (x < 0.0 ? 1.0 - q : q);
    }
    case AGN_ACT_MISH: {
      const double t = tanh(x > 20.0 ? x : log1p(exp(x)));
      return dy * (t + x * sigmoid64(x) * (1.0 - t * t));
    }
    case AGN_ACT_TANHSHRINK: {
      const double t = tanh(x);
      return dy * (t * t);
    }
    default: return x > 0.0 ? dy : 0.0;
  }
}

}  // namespace agn
