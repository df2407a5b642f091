// kernelop.hip — the implicit kernel-matrix operator (rbl_set_matrix_kernel):
//
//     U = (diag(s) K diag(s) + tau I) Q,    K_ij = kappa(x_i, x_j),
//
// from the n x d points alone; K is evaluated tile by tile and never stored.  X lives on the
// device row-major, zero-padded to d4 = 4 ceil(d / 4) columns, beside nrm_i = |x_i|^2
// (kernop_norms: one thread per row, ascending columns).  Distances are taken in Gram form,
// d2_ij = (nrm_i + nrm_j) - 2 x_i.x_j, clamped at 0 and forced to 0 where the global indices
// satisfy i == j (the inner product and the norm are summed in different orders; K_ii is exactly
// 1 for the two radial kernels).  Every term is symmetric in (i, j) bit for bit: the inner product
// runs over k in the same order whichever point is the row, and fp addition commutes.
//
// k_kernop_mfma (16 or 32 columns of Q): a workgroup owns 64 rows i, four waves with one 16-row
// tile each, and walks the column points j in ascending stages of JT points staged through LDS one
// stage ahead (global loads of stage s + 1 are in flight while stage s is computed; two buffers,
// one barrier per stage) and shared by the four waves.  Per 16 x 16 pair tile
//   * d4 / 4 v_mfma_f64_16x16x4_f64 form the TRANSPOSED tile P = X_j X_i^T: A = X_j[l&15][4kk + (l>>4)]
//     from LDS, B = X_i[l&15][4kk + (l>>4)], the wave's fragment, in registers for the whole launch;
//   * the C/D layout (col = l&15, row = (l>>4) + 4 r) puts in register r of lane l the value of
//     row point i = l&15 and column point j = (l>>4) + 4 r — which is the A operand
//     K[i = l&15][k = l>>4] of a second product whose k index runs over j = (l>>4) + 4 r, if its
//     B operand is read as Q_j[(l>>4) + 4 r][l&15].  kappa is applied to the 4 values in place and
//     b / 4 MFMAs add them into the 16 x b output tile; no LDS round trip between the products;
//   * j ascends through r = 0..3 and, inside one MFMA, through its four k: a fixed order.
// s_j multiplies the rows of Q as they are staged, rows of Q past n are staged as zeros (kappa is
// finite for them, so they add exactly 0), the epilogue writes s_i acc + tau Q_i for rows < n.
// Instantiated per fragment capacity KS (1 .. 64 k-steps), 16 / 32 columns and kernel, so kappa
// carries no run-time switch.  Stages of JT = 64 / 32 / 16 points keep a stage's X_j within 16
// prefetch registers per thread and both buffers within 78 KB of LDS.
//
// k_kernop_any (1 to 8 columns): one thread per row, the same ascending j order, plain fma.
//
// No atomics, no scratch; each output element has one owner and one summation order, so two
// applications give the same bits.  kernop_apply serves any width b by column chunks of 32, 16 and
// <= 8 with leading dimension b (the kernel matrix is re-evaluated per chunk).
#include <algorithm>

#include "kernelop_dev.hpp"
#include "kernels.hpp"

namespace rbl {

namespace {

// kern_value, kern_jt and kern_lds_doubles are shared with the cross-kernel product
using namespace kerndev;

__global__ __launch_bounds__(256) void k_kernop_norms(int64_t n, int d4, const double* __restrict__ X,
                                                      double* __restrict__ nrm) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < d4; ++k) {
    const double x = X[i * d4 + k];
    s = fma(x, x, s);
  }
  nrm[i] = s;
}

// KS: the k steps (of 4 columns) the X_i fragment has room for, ks <= KS of them used (ks == KS, d4
// a power of two: the straight-line form with the LDS reads of 8 steps issued ahead of their MFMAs);
// NB: 16-column tiles of Q (the chunk is columns [c0, c0 + 16 NB) of the n x ldq blocks Q and U)
template <int KS, int NB, int KIND>
__global__ __launch_bounds__(256) void k_kernop_mfma(KernOp op, int ks, const double* __restrict__ Q,
                                                     int ldq, int c0, double* __restrict__ U) {
  constexpr int JT = kern_jt(KS);
  constexpr int LDX = JT + 1;            // X_j^T in LDS: element (k, j) at k LDX + j
  constexpr int W = 16 * NB;
  constexpr int XPER = JT * 4 * KS / 256;
  constexpr int QPER = JT * W / 256;
  constexpr int BUF = 4 * KS * LDX + JT * W + JT;
  extern __shared__ double kern_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int64_t n = op.n;
  const int d4 = op.d4;
  const int64_t i0 = (int64_t)blockIdx.x * 64 + 16 * wave;
  const int64_t gi = i0 + li;

  // the wave's X_i fragment (B operand of the first product) and its norm
  double xi[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) xi[kk] = (kk < ks && gi < n) ? op.X[gi * d4 + 4 * kk + q] : 0.0;
  const double ni = gi < n ? op.nrm[gi] : 0.0;

  // where this thread's staged elements of X go (the same every stage)
  const int xcount = JT * d4;
  int xofs[XPER];
#pragma unroll
  for (int m = 0; m < XPER; ++m) {
    const int e = tid + 256 * m;
    xofs[m] = e < xcount ? (e % d4) * LDX + e / d4 : -1;
  }
  double xr[XPER], qr[QPER], nr = 0.0;
  auto load = [&](int64_t j0) {
#pragma unroll
    for (int m = 0; m < XPER; ++m) {
      const int64_t g = j0 * d4 + tid + 256 * m;
      xr[m] = (xofs[m] >= 0 && g < n * d4) ? op.X[g] : 0.0;
    }
#pragma unroll
    for (int m = 0; m < QPER; ++m) {
      const int e = tid + 256 * m;
      const int64_t j = j0 + e / W;
      double v = 0.0;
      if (j < n) {
        v = Q[j * ldq + c0 + e % W];
        if (op.scale) v *= op.scale[j];
      }
      qr[m] = v;
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
  if constexpr (KS >= 64) {  // the X rows past d4 of both buffers, which no stage writes: zero
    for (int e = tid; e < 2 * BUF; e += 256)
      if (e % BUF < 4 * KS * LDX) kern_lds[e] = 0.0;
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
      d4v p = d4v{0.0, 0.0, 0.0, 0.0};
      const double* xt = xs + q * LDX + 16 * t + li;
      if (KS < 64 && ks == KS) {  // (KS = 64: X_i alone fills 128 registers; the guarded form only)
        constexpr int CH = KS < 8 ? KS : 8;
#pragma unroll
        for (int k0 = 0; k0 < KS; k0 += CH) {
          double a[CH];
#pragma unroll
          for (int kk = 0; kk < CH; ++kk) a[kk] = xt[4 * (k0 + kk) * LDX];
#pragma unroll
          for (int kk = 0; kk < CH; ++kk)
            p = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xi[k0 + kk], p, 0, 0, 0);
        }
      } else if constexpr (KS >= 64) {
        // groups of 4 steps under one guard each (64 single guards would not fit the scalar
        // registers): the steps of the last group past ks multiply the zeroed LDS rows by the zero
        // tail of xi and add exact zeros — up to 3 MFMAs more than d4 / 4, for d > 128 only
#pragma unroll
        for (int k0 = 0; k0 < KS; k0 += 4)
          if (k0 < ks) {
            double a[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) a[kk] = xt[4 * (k0 + kk) * LDX];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
              p = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xi[k0 + kk], p, 0, 0, 0);
          }
      } else {
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
          if (kk < ks) p = __builtin_amdgcn_mfma_f64_16x16x4f64(xt[4 * kk * LDX], xi[kk], p, 0, 0, 0);
      }
      double kv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jl = 16 * t + q + 4 * r;
        kv[r] = kern_value<KIND>(op.gamma, op.coef0, op.degree, ni, ns[jl], p[r], gi == j0 + jl);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ct = 0; ct < NB; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[r], qs[(16 * t + q + 4 * r) * W + 16 * ct + li],
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
    const double si = op.scale ? op.scale[row] : 1.0;
#pragma unroll
    for (int ct = 0; ct < NB; ++ct) {
      const int64_t at = row * ldq + c0 + 16 * ct + li;
      U[at] = fma(op.nugget, Q[at], si * acc[ct][r]);
    }
  }
}

// columns [c0, c0 + w), w <= kKernAnyCols, of row i: one thread, j ascending
constexpr int kKernAnyCols = 8;
__global__ __launch_bounds__(64) void k_kernop_any(KernOp op, const double* __restrict__ Q, int ldq, int c0,
                                                   int w, double* __restrict__ U) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t n = op.n;
  if (i >= n) return;
  const int d4 = op.d4;
  const double* xi = op.X + i * d4;
  const double ni = op.nrm[i];
  double acc[kKernAnyCols];
#pragma unroll
  for (int c = 0; c < kKernAnyCols; ++c) acc[c] = 0.0;
  for (int64_t j = 0; j < n; ++j) {
    const double* xj = op.X + j * d4;
    double p = 0.0;
    for (int k = 0; k < d4; ++k) p = fma(xj[k], xi[k], p);
    const double kv = op.kind == kKernRbf       ? kern_value<kKernRbf>(op.gamma, op.coef0, op.degree, ni, op.nrm[j], p, i == j)
                      : op.kind == kKernLaplace ? kern_value<kKernLaplace>(op.gamma, op.coef0, op.degree, ni, op.nrm[j], p, i == j)
                                                : kern_value<kKernPoly>(op.gamma, op.coef0, op.degree, ni, op.nrm[j], p, i == j);
    const double sj = op.scale ? op.scale[j] : 1.0;
    const double* qj = Q + j * ldq + c0;
#pragma unroll
    for (int c = 0; c < kKernAnyCols; ++c)
      if (c < w) acc[c] = fma(kv, op.scale ? sj * qj[c] : qj[c], acc[c]);
  }
  const double si = op.scale ? op.scale[i] : 1.0;
#pragma unroll
  for (int c = 0; c < kKernAnyCols; ++c)
    if (c < w) U[i * ldq + c0 + c] = fma(op.nugget, Q[i * ldq + c0 + c], si * acc[c]);
}

template <int KS, int NB, int KIND>
void launch_mfma_kind(const KernOp& op, const double* Q, int ldq, int c0, double* U, hipStream_t s) {
  constexpr int lds = kern_lds_doubles(KS, NB) * (int)sizeof(double);
  ensure_lds_attr(reinterpret_cast<const void*>(&k_kernop_mfma<KS, NB, KIND>), lds);
  const unsigned grid = (unsigned)ceil_div(op.n, 64);
  hipLaunchKernelGGL((k_kernop_mfma<KS, NB, KIND>), dim3(grid), dim3(256), lds, s, op, op.d4 / 4, Q, ldq, c0, U);
}
template <int KS, int NB>
void launch_mfma(const KernOp& op, const double* Q, int ldq, int c0, double* U, hipStream_t s) {
  if (op.kind == kKernRbf) launch_mfma_kind<KS, NB, kKernRbf>(op, Q, ldq, c0, U, s);
  else if (op.kind == kKernLaplace) launch_mfma_kind<KS, NB, kKernLaplace>(op, Q, ldq, c0, U, s);
  else launch_mfma_kind<KS, NB, kKernPoly>(op, Q, ldq, c0, U, s);
}

template <int NB>
void launch_mfma_ks(const KernOp& op, const double* Q, int ldq, int c0, double* U, hipStream_t s) {
  const int ks = op.d4 / 4;
  if (ks <= 1) launch_mfma<1, NB>(op, Q, ldq, c0, U, s);
  else if (ks <= 2) launch_mfma<2, NB>(op, Q, ldq, c0, U, s);
  else if (ks <= 4) launch_mfma<4, NB>(op, Q, ldq, c0, U, s);
  else if (ks <= 8) launch_mfma<8, NB>(op, Q, ldq, c0, U, s);
  else if (ks <= 16) launch_mfma<16, NB>(op, Q, ldq, c0, U, s);
  else if (ks <= 32) launch_mfma<32, NB>(op, Q, ldq, c0, U, s);
  else launch_mfma<64, NB>(op, Q, ldq, c0, U, s);
}

}  // namespace

void kernop_norms(int64_t n, int d4, const double* X, double* nrm, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_kernop_norms, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, n, d4, X, nrm);
}

bool kernop_apply(const KernOp& op, const double* Q, int b, double* U, hipStream_t s) {
  if (op.n <= 0 || b < 1 || op.d4 < 4 || op.d4 > kKernMaxDim || (op.d4 & 3) || !op.X || !op.nrm) return false;
  if (op.n * (int64_t)std::max(op.d4, b) >= (int64_t)1 << 40) return false;
  int c0 = 0;
  for (; b - c0 >= 32; c0 += 32) launch_mfma_ks<2>(op, Q, b, c0, U, s);
  for (; b - c0 >= 16; c0 += 16) launch_mfma_ks<1>(op, Q, b, c0, U, s);
  for (; c0 < b; c0 += kKernAnyCols)
    hipLaunchKernelGGL(k_kernop_any, dim3((unsigned)ceil_div(op.n, 64)), dim3(64), 0, s, op, Q, b, c0,
                       std::min(kKernAnyCols, b - c0), U);
  return true;
}

}  // namespace rbl
