// kernelop_dev.hpp — what kernelop.hip (the symmetric kernel matrix) and kernelop_cross.hip (the
// rectangular cross-kernel product) share on the device: the kernel function on a Gram-form inner
// product, and the stage geometry of the pair-tile scheme.
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

// column points per stage: 4 KS JT doubles of X and 16 NB JT of Q per buffer
constexpr int kern_jt(int KS) { return KS <= 4 ? 64 : KS <= 16 ? 32 : 16; }
constexpr int kern_lds_doubles(int KS, int NB) {
  return 2 * (4 * KS * (kern_jt(KS) + 1) + kern_jt(KS) * 16 * NB + kern_jt(KS));
}
// the fragment capacity (k steps of 4 columns) the kernels are instantiated for
constexpr int kern_ks_cap(int ks) { return ks <= 1 ? 1 : ks <= 2 ? 2 : ks <= 4 ? 4 : ks <= 8 ? 8 : ks <= 16 ? 16 : ks <= 32 ? 32 : 64; }

}  // namespace kerndev
}  // namespace rbl
