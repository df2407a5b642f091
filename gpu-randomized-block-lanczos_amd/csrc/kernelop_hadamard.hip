// kernelop_hadamard.hip — kernel-matrix derivative products (rbl_kernel_hadamard):
//
//     U = (Phi o A B^T) Q,    Phi_ij = phi(x_i, x_j),    (A B^T)_ij = a_i . b_j,
//
// over the n points of the symmetric operator (kernelop.hip); phi is kappa or one of its derivatives
// (kernelop_dev.hpp, phi<KIND>).  A and B are n x r, row-major and zero-padded to r4 = 4 ceil(r / 4)
// columns; Q and U are n x b row-major with leading dimension b.  Neither the operator's scale nor
// its nugget enters.
//
// k_kernop_hadamard is the pair-tile scheme of k_kernop_mfma with one more Gram-form inner product:
// a column point is the wide row [x_j | b_j] of d4 + r4 doubles, the wave's fragment is [x_i | a_i],
// and of the kt = ks + rs k-steps (ks = d4 / 4, rs = r4 / 4) of a 16 x 16 pair tile the first ks
// accumulate the transposed tile P = X_j X_i^T and the next rs a second tile M = B_j A_i^T in the
// same C/D layout (register r of lane l: row point i = l & 15, column point j = (l >> 4) + 4 r).
// w[r] = phi(...)[r] m[r] is then the A operand of the b / 4 MFMAs with the staged Q_j, exactly as
// kappa is in k_kernop_mfma.  The fragment capacity KS is kern_ks_cap(kt) and the stage length
// kern_jt(KS), so d4 + r4 <= kKernMaxDim.  The X part of P runs through the same instructions in
// the same order as in k_kernop_mfma: with A = B = 1 (m_ij = 1 exactly) and phi = kappa the result
// has the bits of the symmetric operator without scale and nugget, for b a multiple of 16.
//
// The weight mode is a wave-uniform run-time switch (one scalar branch beside an exp), not a
// template parameter: 42 instantiations (7 capacities x 2 widths x 3 kernels) instead of 126.
//
// Any width runs on MFMA: column chunks of 32, and a last chunk of 17 .. 31 columns staged zero-padded
// into 32 or of 1 .. 16 into 16, of which only the real columns are written (Phi o A B^T is evaluated
// once per chunk, so b = 17 is one launch; a multiple of 16 runs in kernop_apply's chunks).  The column range
// is not split: the grid is ceil(n / 64), j ascends through the stages, t, r and the four k of one
// MFMA.  No atomics, no scratch; each output element has one owner and one summation order.
#include <algorithm>

#include "kernelop_dev.hpp"
#include "kernels.hpp"

namespace rbl {

namespace {

using namespace kerndev;

// NB: 16-column tiles of the chunk [c0, c0 + wc), wc <= 16 NB real columns (the rest staged as zeros
// and not written).  ks + rs <= KS k-steps are used: ks of X, then rs of A / B (r4 = 4 rs).
// (two waves per SIMD up to KS = 16, where the fragment leaves room for them: a workgroup's four waves
// then share a CU with a second workgroup's)
template <int KS, int NB, int KIND>
__global__ __launch_bounds__(256, KS <= 16 ? 2 : 1) void k_kernop_hadamard(KernOp op, int ks, int rs, int mode,
                                                         const double* __restrict__ Ap,
                                                         const double* __restrict__ Bp,
                                                         const double* __restrict__ Q, int ldq, int c0, int wc,
                                                         double* __restrict__ U) {
  constexpr int JT = kern_jt(KS);
  constexpr int LDX = JT + 1;            // [X_j | B_j]^T in LDS: element (k, j) at k LDX + j
  constexpr int W = 16 * NB;
  constexpr int XPER = JT * 4 * KS / 256;
  constexpr int QPER = JT * W / 256;
  constexpr int BUF = 4 * KS * LDX + JT * W + JT;
  extern __shared__ double kern_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int64_t n = op.n;
  const int d4 = op.d4, r4 = 4 * rs, kt = ks + rs, dw = d4 + r4;
  const int64_t i0 = (int64_t)blockIdx.x * 64 + 16 * wave;
  const int64_t gi = i0 + li;

  // the wave's [x_i | a_i] fragment (B operand of the two first products) and the norm of x_i
  double xi[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    double v = 0.0;
    if (gi < n) {
      if (kk < ks) v = op.X[gi * d4 + 4 * kk + q];
      else if (kk < kt) v = Ap[gi * r4 + 4 * (kk - ks) + q];
    }
    xi[kk] = v;
  }
  const double ni = gi < n ? op.nrm[gi] : 0.0;

  // where this thread's staged elements of the wide rows go and come from (the same every stage):
  // xofs the LDS offset (-1: none); xsrc >= 0 the offset in X of stage point 0, < 0: -(1 + that in B)
  int xofs[XPER], xsrc[XPER];
#pragma unroll
  for (int m = 0; m < XPER; ++m) {
    const int e = tid + 256 * m;
    const int j = e / dw, k = e % dw;
    xofs[m] = e < JT * dw ? k * LDX + j : -1;
    xsrc[m] = k < d4 ? j * d4 + k : -(1 + j * r4 + (k - d4));
  }
  double xr[XPER], qr[QPER], nr = 0.0;
  auto load = [&](int64_t j0) {
#pragma unroll
    for (int m = 0; m < XPER; ++m) {
      double v = 0.0;
      if (xofs[m] >= 0) {
        if (xsrc[m] >= 0) {
          const int64_t g = j0 * d4 + xsrc[m];
          if (g < n * d4) v = op.X[g];
        } else {
          const int64_t g = j0 * r4 + (-1 - xsrc[m]);
          if (g < n * r4) v = Bp[g];
        }
      }
      xr[m] = v;
    }
#pragma unroll
    for (int m = 0; m < QPER; ++m) {
      const int e = tid + 256 * m;
      const int64_t j = j0 + e / W;
      const int c = e % W;
      qr[m] = (j < n && c < wc) ? Q[j * ldq + c0 + c] : 0.0;
    }
    if (tid < JT) nr = j0 + tid < n ? op.nrm[j0 + tid] : 0.0;
  };
  auto store = [&](double* buf) {
    double* xs = buf;
    double* qs = buf + 4 * KS * LDX;
    double* ns = qs + JT * W;
#pragma unroll
    for (int m = 0; m < XPER; ++m)
      if (xofs[m] >= 0) xs[xofs[m]] = xr[m];
#pragma unroll
    for (int m = 0; m < QPER; ++m) qs[tid + 256 * m] = qr[m];
    if (tid < JT) ns[tid] = nr;
  };

  d4v acc[NB];
#pragma unroll
  for (int ct = 0; ct < NB; ++ct) acc[ct] = d4v{0.0, 0.0, 0.0, 0.0};

  const int64_t nst = (n + JT - 1) / JT;
  if (kt < KS) {  // the wide-row elements past d4 + r4 of both buffers, which no stage writes: zero
    for (int e = tid; e < 2 * BUF; e += 256)
      if (e % BUF >= dw * LDX && e % BUF < 4 * KS * LDX) kern_lds[e] = 0.0;
    __syncthreads();
  }
  load(0);
  store(kern_lds);
  __syncthreads();
  for (int64_t s = 0; s < nst; ++s) {
    const int64_t j0 = s * JT;
    if (s + 1 < nst) load(j0 + JT);
    const double* buf = kern_lds + (s & 1) * BUF;
    const double* xs = buf;
    const double* qs = buf + 4 * KS * LDX;
    const double* ns = qs + JT * W;
#pragma unroll
    for (int t = 0; t < JT / 16; ++t) {
      if (j0 + 16 * t >= n) break;  // a pair tile wholly past n adds exact zeros
      d4v p = d4v{0.0, 0.0, 0.0, 0.0}, mm = d4v{0.0, 0.0, 0.0, 0.0};
      const double* xt = xs + q * LDX + 16 * t + li;
      // groups of G steps under wave-uniform guards, the LDS reads of a group issued ahead of its
      // MFMAs: a group wholly inside the X part chains on p, one wholly inside the A / B part on m,
      // and the one group that holds the boundary decides per step.  Steps of the last group past
      // kt multiply the zeroed LDS rows by the zero tail of the fragment and add exact zeros to m.
      constexpr int G = KS < 8 ? KS : 8;
#pragma unroll
      for (int k0 = 0; k0 < KS; k0 += G)
        if (k0 < kt) {
          double a[G];
#pragma unroll
          for (int kk = 0; kk < G; ++kk) a[kk] = xt[4 * (k0 + kk) * LDX];
          if (k0 + G <= ks) {
#pragma unroll
            for (int kk = 0; kk < G; ++kk) p = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xi[k0 + kk], p, 0, 0, 0);
          } else if (k0 >= ks) {
#pragma unroll
            for (int kk = 0; kk < G; ++kk) mm = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xi[k0 + kk], mm, 0, 0, 0);
          } else {
#pragma unroll
            for (int kk = 0; kk < G; ++kk) {
              if (k0 + kk < ks) p = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xi[k0 + kk], p, 0, 0, 0);
              else mm = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xi[k0 + kk], mm, 0, 0, 0);
            }
          }
        }
      double w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jl = 16 * t + q + 4 * r;
        w[r] = phi<KIND>(mode, op.gamma, op.coef0, op.degree, ni, ns[jl], p[r], gi == j0 + jl) * mm[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ct = 0; ct < NB; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[r], qs[(16 * t + q + 4 * r) * W + 16 * ct + li],
                                                         acc[ct], 0, 0, 0);
    }
    if (s + 1 < nst) store(kern_lds + ((s + 1) & 1) * BUF);
    __syncthreads();
  }

  // acc[ct][r]: row i0 + q + 4 r, column c0 + 16 ct + li
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = i0 + q + 4 * r;
    if (row >= n) continue;
#pragma unroll
    for (int ct = 0; ct < NB; ++ct)
      if (16 * ct + li < wc) U[row * ldq + c0 + 16 * ct + li] = acc[ct][r];
  }
}

struct HadArgs {
  int mode, rs;
  const double *Ap, *Bp, *Q;
  int ldq, c0, wc;
  double* U;
};

template <int KS, int NB, int KIND>
void launch_kind(const KernOp& op, const HadArgs& a, hipStream_t s) {
  constexpr int lds = kern_lds_doubles(KS, NB) * (int)sizeof(double);
  ensure_lds_attr(reinterpret_cast<const void*>(&k_kernop_hadamard<KS, NB, KIND>), lds);
  const unsigned grid = (unsigned)ceil_div(op.n, 64);
  hipLaunchKernelGGL((k_kernop_hadamard<KS, NB, KIND>), dim3(grid), dim3(256), lds, s, op, op.d4 / 4, a.rs,
                     a.mode, a.Ap, a.Bp, a.Q, a.ldq, a.c0, a.wc, a.U);
}
template <int KS, int NB>
void launch(const KernOp& op, const HadArgs& a, hipStream_t s) {
  if (op.kind == kKernRbf) launch_kind<KS, NB, kKernRbf>(op, a, s);
  else if (op.kind == kKernLaplace) launch_kind<KS, NB, kKernLaplace>(op, a, s);
  else launch_kind<KS, NB, kKernPoly>(op, a, s);
}
template <int NB>
void launch_ks(const KernOp& op, const HadArgs& a, hipStream_t s) {
  switch (kern_ks_cap(op.d4 / 4 + a.rs)) {
    case 1: return launch<1, NB>(op, a, s);  // (never: ks >= 1 and rs >= 1)
    case 2: return launch<2, NB>(op, a, s);
    case 4: return launch<4, NB>(op, a, s);
    case 8: return launch<8, NB>(op, a, s);
    case 16: return launch<16, NB>(op, a, s);
    case 32: return launch<32, NB>(op, a, s);
    default: return launch<64, NB>(op, a, s);
  }
}

}  // namespace

bool kernop_hadamard(const KernOp& op, int mode, int r4, const double* Ap, const double* Bp, const double* Q,
                     int b, double* U, hipStream_t s) {
  if (op.n <= 0 || b < 1 || op.d4 < 4 || (op.d4 & 3) || r4 < 4 || (r4 & 3) || op.d4 + r4 > kKernMaxDim || !op.X ||
      !op.nrm || !Ap || !Bp || !Q || !U)
    return false;
  if (mode != kKernWeightValue && mode != kKernWeightDgamma && mode != kKernWeightDscale) return false;
  if (op.n * (int64_t)std::max(op.d4 + r4, b) >= (int64_t)1 << 40) return false;
  HadArgs a{mode, r4 / 4, Ap, Bp, Q, b, 0, 0, U};
  // chunks of 32 columns, the last one of 17 .. 31 zero-padded to 32 (one evaluation of Phi o A B^T
  // instead of two) or of 1 .. 16 to 16; a multiple of 16 runs as kernop_apply's chunks do
  for (; a.c0 < b; a.c0 += a.wc) {
    a.wc = std::min(32, b - a.c0);
    if (a.wc > 16) launch_ks<2>(op, a, s);
    else launch_ks<1>(op, a, s);
  }
  return true;
}

}  // namespace rbl
