// kernelop_dev.hpp — what kernelop.hip (the symmetric kernel matrix), kernelop_cross.hip (the
// rectangular cross-kernel product) and kernelop_hadamard.hip (the derivative products) share on the
// device: the kernel function and its derivatives on a Gram-form inner product, and the stage
// geometry of the pair-tile scheme.
#pragma once

#include "kernels.hpp"

namespace rbl {
namespace kerndev {

typedef double d4v __attribute__((ext_vector_type(4)));

// kappa from the inner product p = x_i.x_j and the squared norms ni, nj; `same`: the two points are
// one point of one set (the diagonal rule of the symmetric operator; the cross product passes false)
template <int KIND>
__device__ __forceinline__ double kern_value(double gamma, double coef0, int degree, double ni, double nj,
                                              double p, bool same) {
  if constexpr (KIND == kKernPoly) {
    const double t = fma(gamma, p, coef0);
    double r = t;
    for (int q = 1; q < degree; ++q) r *= t;
    return r;
  }
  double d2 = fmax((ni + nj) - 2.0 * p, 0.0);
  if (same) d2 = 0.0;
  return exp(-gamma * (KIND == kKernRbf ? d2 : sqrt(d2)));
}

// phi: kappa (mode kKernWeightValue, the bits of kern_value) or the factor of one of its derivatives,
// from the same p, ni, nj and diagonal rule; d2 and t = gamma p + c0 as in kern_value, q = degree:
//   kKernWeightDgamma  d kappa / d gamma:   rbf -d2 kappa   laplace -sqrt(d2) kappa   poly q p t^(q-1)
//   kKernWeightDscale  psi with d kappa / d log s_k = psi (x_ik - x_jk)^2 (radial), psi x_ik x_jk (poly),
//                      at unit coordinate scales:
//                                           rbf -2 gamma kappa
//                                           laplace -gamma kappa / sqrt(d2), 0 where d2 == 0
//                                           poly 2 q gamma t^(q-1)
// mode is wave-uniform (a kernel argument): one scalar branch.
template <int KIND>
__device__ __forceinline__ double phi(int mode, double gamma, double coef0, int degree, double ni, double nj,
                                      double p, bool same) {
  if (mode == kKernWeightValue) return kern_value<KIND>(gamma, coef0, degree, ni, nj, p, same);
  if constexpr (KIND == kKernPoly) {
    const double t = fma(gamma, p, coef0);
    double r = 1.0;  // t^(q-1)
    for (int q = 1; q < degree; ++q) r *= t;
    return mode == kKernWeightDgamma ? (double)degree * p * r : 2.0 * (double)degree * gamma * r;
  }
  double d2 = fmax((ni + nj) - 2.0 * p, 0.0);
  if (same) d2 = 0.0;
  if constexpr (KIND == kKernRbf) {
    const double k = exp(-gamma * d2);
    return mode == kKernWeightDgamma ? -d2 * k : -2.0 * gamma * k;
  }
  const double sd = sqrt(d2);
  const double k = exp(-gamma * sd);
  if (mode == kKernWeightDgamma) return -sd * k;
  return d2 == 0.0 ? 0.0 : -gamma * k / sd;
}

// column points per stage: 4 KS JT doubles of X and 16 NB JT of Q per buffer
constexpr int kern_jt(int KS) { return KS <= 4 ? 64 : KS <= 16 ? 32 : 16; }
constexpr int kern_lds_doubles(int KS, int NB) {
  return 2 * (4 * KS * (kern_jt(KS) + 1) + kern_jt(KS) * 16 * NB + kern_jt(KS));
}
// the fragment capacity (k steps of 4 columns) the kernels are instantiated for
constexpr int kern_ks_cap(int ks) { return ks <= 1 ? 1 : ks <= 2 ? 2 : ks <= 4 ? 4 : ks <= 8 ? 8 : ks <= 16 ? 16 : ks <= 32 ? 32 : 64; }

}  // namespace kerndev
}  // namespace rbl
