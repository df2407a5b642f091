// spmm_cheb.hip — the row passes of the Chebyshev-filtered operator and of Rayleigh-Ritz on A
// (gfx950).
//
// The filter p(A) = T_d((A - cI)/e) / T_d((ref - c)/e) is applied by the scaled three-term
// recurrence of Zhou and Saad (rbl_api.cpp cheb_apply): every term is one SpMM W = A Y_{j-1}
// through whichever SpMM kernel the matrix runs, followed by ONE pass of cheb_axpby
//
//     Y_j = alpha W + beta Y_{j-1} (+ gamma Y_{j-2})
//
// over the n x b row-major blocks.  The blocks are contiguous (leading dimension b), so the
// pass is a flat stream: 16-byte loads and stores when every block starts on a 16-byte boundary
// (a basis slot starts at a multiple of n_local * b doubles, so an odd n_local * b leaves slots
// 8-byte aligned: then the 8-byte form runs), a guarded last element when n * b is odd, and a
// grid sized from the CU count, each thread walking the stream grid-stride.  Y_j may be written
// over W (each thread reads an element of W before it writes it).
//
// cheb_series_term is the row pass of a general Chebyshev series sum_j mu_j T_j((A - cI)/e)
// (rbl_set_filter_series; rbl_api.cpp series_apply): the unscaled recurrence term and the
// accumulation into the result in one sweep — 4 reads + 2 writes per element (W, T_{j-1},
// T_{j-2}, ACC; T_j, ACC) against the 5 + 2 of cheb_axpby followed by a second cheb_axpby as
// the accumulate, and one launch instead of two.
//
// cheb_moment_term is the row pass of the Chebyshev moments x^T T_j((A - cI)/e) x
// (rbl_cheb_moments): the same unscaled term, and in the same sweep the per-column partial sums
// of <t_j,t_j> and <t_j,t_{j-1}> — 3 reads + 1 write per element, no second sweep for the dots,
// the sums in the fixed order of resid_partial.
//
// cheb_diag_term is the row pass of the diagonals of nf Chebyshev series at once (rbl_cheb_diag:
// diag f(A) by probing): the same unscaled term, and in the same sweep the sums ALONG each row
// over the b probe columns, s[row] = sum_c X[row][c] t_j[row][c], added into nf accumulators per
// row with the term's coefficients — 4 reads + 1 write per element plus 16 nf / b bytes for D, one
// recurrence for all nf functions.  sign_block turns a block into its signs (Rademacher probes).
//
// resid_partial forms the per-workgroup partials of the column sums of (Z - X diag(theta))^2 —
// the true residuals ||A v - theta v||^2 of rbl_ritz_finish — summed in a fixed order (each
// thread over its rows ascending, then the workgroup's row groups ascending in LDS; reduce_slab
// adds the workgroups in order): no float atomics, the same bits on every run.
//
// copy_cols moves a column range between row-major blocks of different widths (the column
// chunks rbl_ritz_project multiplies by A).
#include <algorithm>
#include <mutex>

#include "kernels.hpp"

namespace rbl {

namespace {

constexpr int kChebThreads = 256;
constexpr int kChebPerCu = 8;    // workgroups per CU of the stream pass (2 waves per SIMD x 4)
constexpr int kResidPerCu = 4;
constexpr int kResidMinRows = 64;  // rows per workgroup below which a smaller grid runs

int cu_count() {
  static std::mutex mu;
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  std::lock_guard<std::mutex> g(mu);
  if (cus[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
      v = 256;
    cus[dev] = v;
  }
  return cus[dev];
}

// T = d2v: pairs (16 B), T = double: single elements.  npk: elements of type T; tail: one last
// double past the pairs (or -1).
template <typename T, bool HAS_Z>
__global__ __launch_bounds__(kChebThreads) void k_cheb_axpby(int64_t npk, int64_t tail, const T* W,
                                                             const T* __restrict__ Y,
                                                             const T* __restrict__ Z, double alpha,
                                                             double beta, double gamma, T* out) {
  const int64_t stride = (int64_t)gridDim.x * kChebThreads;
  for (int64_t i = (int64_t)blockIdx.x * kChebThreads + threadIdx.x; i < npk; i += stride) {
    T r = alpha * W[i] + beta * Y[i];
    if constexpr (HAS_Z) r += gamma * Z[i];
    out[i] = r;
  }
  if (tail >= 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    const double* w = reinterpret_cast<const double*>(W);
    const double* y = reinterpret_cast<const double*>(Y);
    double r = alpha * w[tail] + beta * y[tail];
    if constexpr (HAS_Z) r += gamma * reinterpret_cast<const double*>(Z)[tail];
    reinterpret_cast<double*>(out)[tail] = r;
  }
}

// One term of the Chebyshev series out = sum_j mu_j T_j (rbl_set_filter_series) after its SpMM
// W = A T_{j-1}, the same stream conventions as k_cheb_axpby:
//     T_j = alpha W + beta T_{j-1} (- T_{j-2}),   ACC (+)= mu_j T_j.
// FIRST (j = 1): T_{j-1} = X, no T_{j-2}, and ACC = mu_0 X + mu_1 T_1 (ACC is not read).
// LAST (j = d): T_d is not stored.  Tout may be W (each thread reads W[i] before it writes it);
// ACC is distinct from every other block.
template <typename T, bool FIRST, bool LAST>
__global__ __launch_bounds__(kChebThreads) void k_cheb_series(int64_t npk, int64_t tail, const T* W,
                                                              const T* __restrict__ T1,
                                                              const T* __restrict__ T2, double alpha,
                                                              double beta, double mu, double mu0,
                                                              T* Tout, T* __restrict__ ACC) {
  const int64_t stride = (int64_t)gridDim.x * kChebThreads;
  for (int64_t i = (int64_t)blockIdx.x * kChebThreads + threadIdx.x; i < npk; i += stride) {
    const T t1 = T1[i];
    T t = alpha * W[i] + beta * t1;
    if constexpr (FIRST) {
      ACC[i] = mu0 * t1 + mu * t;
    } else {
      t -= T2[i];
      ACC[i] += mu * t;
    }
    if constexpr (!LAST) Tout[i] = t;
  }
  if (tail >= 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    const double t1 = reinterpret_cast<const double*>(T1)[tail];
    double t = alpha * reinterpret_cast<const double*>(W)[tail] + beta * t1;
    double* acc = reinterpret_cast<double*>(ACC);
    if constexpr (FIRST) {
      acc[tail] = mu0 * t1 + mu * t;
    } else {
      t -= reinterpret_cast<const double*>(T2)[tail];
      acc[tail] += mu * t;
    }
    if constexpr (!LAST) reinterpret_cast<double*>(Tout)[tail] = t;
  }
}

template <typename T>
void launch_cheb_series(int grid, int64_t npk, int64_t tail, const double* W, const double* T1,
                        const double* T2, double alpha, double beta, double mu, double mu0,
                        double* Tout, double* ACC, bool first, bool last, hipStream_t s) {
  const T *w = reinterpret_cast<const T*>(W), *t1 = reinterpret_cast<const T*>(T1),
          *t2 = reinterpret_cast<const T*>(T2);
  T *to = reinterpret_cast<T*>(Tout), *acc = reinterpret_cast<T*>(ACC);
#define RBL_SERIES_LAUNCH(F, L)                                                                    \
  hipLaunchKernelGGL((k_cheb_series<T, F, L>), dim3(grid), dim3(kChebThreads), 0, s, npk, tail, w, \
                     t1, t2, alpha, beta, mu, mu0, to, acc)
  if (first && last) RBL_SERIES_LAUNCH(true, true);
  else if (first) RBL_SERIES_LAUNCH(true, false);
  else if (last) RBL_SERIES_LAUNCH(false, true);
  else RBL_SERIES_LAUNCH(false, false);
#undef RBL_SERIES_LAUNCH
}

// CW columns x RG row groups per workgroup (CW * RG = 256, CW a power of two >= min(kp, 256))
__global__ __launch_bounds__(kChebThreads) void k_resid_partial(int64_t nrows, int kp, int cw,
                                                                const double* __restrict__ Z,
                                                                const double* __restrict__ X,
                                                                const double* __restrict__ theta,
                                                                double* __restrict__ part) {
  __shared__ double sm[kChebThreads];
  const int rg = threadIdx.x / cw, c0 = threadIdx.x % cw, nrg = kChebThreads / cw;
  const int64_t per = (nrows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per;
  const int64_t r1 = r0 + per < nrows ? r0 + per : nrows;
  auto colsum = [&](int c) {
    const double th = theta[c];
    double acc = 0.0;
    for (int64_t r = r0 + rg; r < r1; r += nrg) {
      const double d = Z[r * kp + c] - X[r * kp + c] * th;
      acc += d * d;
    }
    return acc;
  };
  if (nrg == 1) {  // kp > 128: one thread per column (and per 256 columns), no LDS stage
    for (int c = c0; c < kp; c += cw) part[(int64_t)blockIdx.x * kp + c] = colsum(c);
    return;
  }
  // kp <= cw: one column per thread; every thread reaches the barrier
  sm[threadIdx.x] = c0 < kp ? colsum(c0) : 0.0;
  __syncthreads();
  if (rg == 0 && c0 < kp) {
    double s = 0.0;
    for (int g = 0; g < nrg; ++g) s += sm[g * cw + c0];
    part[(int64_t)blockIdx.x * kp + c0] = s;
  }
}

// One term of the moment recurrence (rbl_cheb_moments) after its SpMM W = A t_{j-1}:
//     t_j = alpha W + beta t_{j-1} (- t_{j-2}),   stored to Tout unless LAST (Tout may be W),
// and the workgroup's partials of the column sums <t_j,t_j>, <t_j,t_{j-1}> and, FIRST (j = 1:
// t_{j-1} = x, no t_{j-2}), <x,x>:  part[g][q][c], q < NQ = 2 (3 if FIRST), c < b.
// A row of the n x b row-major blocks is cw slots of type T (d2v: cw = b / 2 column pairs, double:
// cw = b columns), so a thread keeps its slot's columns for the whole pass.  The workgroup covers
// a tile of nrg = 256 / cw rows at a time (thread t reads slot t of the tile: one contiguous
// stream per workgroup) and the tiles are walked grid-stride; a row wider than 256 slots is
// covered in chunks of 256, one after the other.  The sums keep a fixed order, as
// k_resid_partial's: each thread over its rows ascending, then the row groups ascending in LDS;
// reduce_slab adds the workgroups in order.  No atomics.
template <typename T>
__device__ __forceinline__ void moment_stage(double* sm, int q, T v);
template <>
__device__ __forceinline__ void moment_stage<double>(double* sm, int q, double v) {
  sm[q * kChebThreads + threadIdx.x] = v;
}
template <>
__device__ __forceinline__ void moment_stage<d2v>(double* sm, int q, d2v v) {
  sm[(2 * q) * kChebThreads + threadIdx.x] = v.x;
  sm[(2 * q + 1) * kChebThreads + threadIdx.x] = v.y;
}

template <typename T, bool FIRST, bool LAST>
__global__ __launch_bounds__(kChebThreads) void k_cheb_moment(int64_t nrows, int cw, const T* W,
                                                              const T* __restrict__ T1,
                                                              const T* __restrict__ T2, double alpha,
                                                              double beta, T* Tout,
                                                              double* __restrict__ part) {
  constexpr int VW = sizeof(T) / sizeof(double);  // columns per slot
  constexpr int NQ = FIRST ? 3 : 2;
  __shared__ double sm[NQ * VW * kChebThreads];
  const int cwl = cw < kChebThreads ? cw : kChebThreads;  // slots of a row covered at once
  const int nrg = kChebThreads / cwl;                     // rows per tile
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  double* out = part + (int64_t)blockIdx.x * NQ * VW * cw;
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    T tt = T(0.0), tp = T(0.0), xx = T(0.0);
    if (rg < nrg && c < cw) {
      for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < nrows; r += rstride) {
        const int64_t i = r * cw + c;
        const T t1 = T1[i];
        T t = alpha * W[i] + beta * t1;
        if constexpr (FIRST) xx += t1 * t1;
        else t -= T2[i];
        tt += t * t;
        tp += t * t1;
        if constexpr (!LAST) Tout[i] = t;
      }
    }
    moment_stage<T>(sm, 0, tt);
    moment_stage<T>(sm, 1, tp);
    if constexpr (FIRST) moment_stage<T>(sm, 2, xx);
    __syncthreads();
    const int ncl = cw - cb < cwl ? cw - cb : cwl;  // slots of this chunk
    for (int idx = threadIdx.x; idx < NQ * VW * ncl; idx += kChebThreads) {
      const int qv = idx / ncl, c2 = idx % ncl;  // qv = q * VW + lane of the slot
      double s = 0.0;
      for (int g = 0; g < nrg; ++g) s += sm[qv * kChebThreads + g * cwl + c2];
      out[(qv / VW) * (VW * cw) + (cb + c2) * VW + qv % VW] = s;
    }
    __syncthreads();
  }
}

template <typename T>
void launch_cheb_moment(int grid, int64_t nrows, int cw, const double* W, const double* T1,
                        const double* T2, double alpha, double beta, double* Tout, double* part,
                        bool first, bool last, hipStream_t s) {
  const T *w = reinterpret_cast<const T*>(W), *t1 = reinterpret_cast<const T*>(T1),
          *t2 = reinterpret_cast<const T*>(T2);
  T* to = reinterpret_cast<T*>(Tout);
#define RBL_MOMENT_LAUNCH(F, L)                                                                   \
  hipLaunchKernelGGL((k_cheb_moment<T, F, L>), dim3(grid), dim3(kChebThreads), 0, s, nrows, cw, w, \
                     t1, t2, alpha, beta, to, part)
  if (first && last) RBL_MOMENT_LAUNCH(true, true);
  else if (first) RBL_MOMENT_LAUNCH(true, false);
  else if (last) RBL_MOMENT_LAUNCH(false, true);
  else RBL_MOMENT_LAUNCH(false, false);
#undef RBL_MOMENT_LAUNCH
}

// One term of the diagonal recurrence (rbl_cheb_diag) after its SpMM W = A t_{j-1}: the term of
// k_cheb_moment,
//     t_j = alpha W + beta t_{j-1} (- t_{j-2}),   stored to Tout unless LAST (Tout may be W),
// and in the same sweep the sums ALONG each row over the b probe columns,
//     s[row] = sum_c X[row][c] t_j[row][c],   D[row][e] += coef[e] s[row],  e < nf
// (coef: the nf coefficients of this term; D: n x nf row-major).  FIRST (j = 1: t_{j-1} = X, T1 and
// T2 are not read, coef holds the 2 nf coefficients of terms 0 and 1): also q[row] = sum_c X^2,
// qout[row] = q and D[row][e] = coef[e] q + coef[nf + e] s — D is not read.
// The thread mapping is k_cheb_moment's: a row is cw <= 256 slots of type T, the workgroup covers
// a tile of nrg = 256 / cw whole rows (thread t reads slot t of the tile), tiles are walked
// grid-stride.  A row never leaves its tile pass (b <= 256), so there is no cross-chunk
// accumulation: each thread stages its slot's products in LDS, and the thread that owns (row, e)
// adds the row's slots ascending and does the read-modify-write of D.  No atomics, one owner per
// element of D: the same bits on every run.  The LDS stage is double-buffered, one barrier per
// tile (a buffer is rewritten two tiles later, after the barrier of the tile between).
template <typename T>
__device__ __forceinline__ double slot_dot(T a, T b);
template <>
__device__ __forceinline__ double slot_dot<double>(double a, double b) {
  return a * b;
}
template <>
__device__ __forceinline__ double slot_dot<d2v>(d2v a, d2v b) {
  return a.x * b.x + a.y * b.y;
}

template <typename T, bool FIRST, bool LAST>
__global__ __launch_bounds__(kChebThreads) void k_cheb_diag(int64_t nrows, int cw, int nf, const T* W,
                                                            const T* __restrict__ T1,
                                                            const T* __restrict__ T2,
                                                            const T* __restrict__ X, double alpha,
                                                            double beta, T* Tout,
                                                            const double* __restrict__ coef,
                                                            double* __restrict__ D,
                                                            double* __restrict__ qout) {
  constexpr int NQ = FIRST ? 2 : 1;
  __shared__ double sm[2][NQ][kChebThreads];
  const int nrg = kChebThreads / cw;  // rows per tile (cw <= 256)
  const int rg = threadIdx.x / cw, cl = threadIdx.x % cw;
  const int64_t ntiles = (nrows + nrg - 1) / nrg;
  int buf = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    const int64_t r0 = tile * nrg, r = r0 + rg;
    double s = 0.0, q = 0.0;
    if (rg < nrg && r < nrows) {
      const int64_t i = r * cw + cl;
      const T x = X[i];
      T t;
      if constexpr (FIRST) {
        t = alpha * W[i] + beta * x;
        q = slot_dot<T>(x, x);
      } else {
        t = alpha * W[i] + beta * T1[i];
        t -= T2[i];
      }
      s = slot_dot<T>(x, t);
      if constexpr (!LAST) Tout[i] = t;
    }
    sm[buf][0][threadIdx.x] = s;
    if constexpr (FIRST) sm[buf][1][threadIdx.x] = q;
    __syncthreads();
    const int64_t left = nrows - r0;
    const int rows = left < nrg ? (int)left : nrg;
    for (int idx = threadIdx.x; idx < rows * nf; idx += kChebThreads) {
      const int g = idx / nf, e = idx - g * nf;
      const double* ps = &sm[buf][0][g * cw];
      double rs = 0.0;
      for (int c = 0; c < cw; ++c) rs += ps[c];
      const int64_t di = r0 * nf + idx;  // = (r0 + g) * nf + e
      if constexpr (FIRST) {
        const double* pq = &sm[buf][1][g * cw];
        double rq = 0.0;
        for (int c = 0; c < cw; ++c) rq += pq[c];
        D[di] = coef[e] * rq + coef[nf + e] * rs;
        if (e == 0) qout[r0 + g] = rq;
      } else {
        D[di] += coef[e] * rs;
      }
    }
  }
}

template <typename T>
void launch_cheb_diag(int grid, int64_t nrows, int cw, int nf, const double* W, const double* T1,
                      const double* T2, const double* X, double alpha, double beta, double* Tout,
                      const double* coef, double* D, double* qout, bool first, bool last,
                      hipStream_t s) {
  const T *w = reinterpret_cast<const T*>(W), *t1 = reinterpret_cast<const T*>(T1),
          *t2 = reinterpret_cast<const T*>(T2), *x = reinterpret_cast<const T*>(X);
  T* to = reinterpret_cast<T*>(Tout);
#define RBL_DIAG_LAUNCH(F, L)                                                                       \
  hipLaunchKernelGGL((k_cheb_diag<T, F, L>), dim3(grid), dim3(kChebThreads), 0, s, nrows, cw, nf, w, \
                     t1, t2, x, alpha, beta, to, coef, D, qout)
  if (first && last) RBL_DIAG_LAUNCH(true, true);
  else if (first) RBL_DIAG_LAUNCH(true, false);
  else if (last) RBL_DIAG_LAUNCH(false, true);
  else RBL_DIAG_LAUNCH(false, false);
#undef RBL_DIAG_LAUNCH
}

// x = +1 where x >= 0 (0 and -0 included), -1 where x < 0, in place: the signs of the N(0,1) draw
// are a Rademacher block (rbl_cheb_diag with RBL_PROBE_SIGN).
__global__ __launch_bounds__(kChebThreads) void k_sign_block(int64_t len, double* x) {
  const int64_t stride = (int64_t)gridDim.x * kChebThreads;
  for (int64_t i = (int64_t)blockIdx.x * kChebThreads + threadIdx.x; i < len; i += stride)
    x[i] = x[i] < 0.0 ? -1.0 : 1.0;
}

__global__ __launch_bounds__(kChebThreads) void k_copy_cols(int64_t nrows, int w, const double* __restrict__ src,
                                                            int lds, int s0, double* __restrict__ dst,
                                                            int ldd, int d0) {
  const int64_t total = nrows * w, stride = (int64_t)gridDim.x * kChebThreads;
  for (int64_t i = (int64_t)blockIdx.x * kChebThreads + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / w;
    const int c = (int)(i - r * w);
    dst[r * ldd + d0 + c] = src[r * lds + s0 + c];
  }
}

int stream_grid(int64_t work_items, int per_cu) {
  const int64_t want = (work_items + kChebThreads - 1) / kChebThreads;
  const int64_t cap = (int64_t)cu_count() * per_cu;
  return (int)std::max<int64_t>(1, std::min(want, cap));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void cheb_axpby(int64_t len, const double* W, const double* Y, const double* Z, double alpha,
                double beta, double gamma, double* out, hipStream_t s) {
  if (len <= 0) return;
  const bool vec = aligned16(W) && aligned16(Y) && aligned16(out) && (!Z || aligned16(Z));
  if (vec) {
    const int64_t np = len / 2, tail = (len & 1) ? len - 1 : -1;
    const int grid = stream_grid(np, kChebPerCu);
    const d2v *w = reinterpret_cast<const d2v*>(W), *y = reinterpret_cast<const d2v*>(Y);
    d2v* o = reinterpret_cast<d2v*>(out);
    if (Z)
      hipLaunchKernelGGL((k_cheb_axpby<d2v, true>), dim3(grid), dim3(kChebThreads), 0, s, np, tail, w, y,
                         reinterpret_cast<const d2v*>(Z), alpha, beta, gamma, o);
    else
      hipLaunchKernelGGL((k_cheb_axpby<d2v, false>), dim3(grid), dim3(kChebThreads), 0, s, np, tail, w, y,
                         static_cast<const d2v*>(nullptr), alpha, beta, gamma, o);
    return;
  }
  const int grid = stream_grid(len, kChebPerCu);
  if (Z)
    hipLaunchKernelGGL((k_cheb_axpby<double, true>), dim3(grid), dim3(kChebThreads), 0, s, len,
                       (int64_t)-1, W, Y, Z, alpha, beta, gamma, out);
  else
    hipLaunchKernelGGL((k_cheb_axpby<double, false>), dim3(grid), dim3(kChebThreads), 0, s, len,
                       (int64_t)-1, W, Y, static_cast<const double*>(nullptr), alpha, beta, gamma, out);
}

void cheb_series_term(int64_t len, const double* W, const double* T1, const double* T2, double alpha,
                      double beta, double mu, double mu0, double* Tout, double* ACC, bool first,
                      bool last, hipStream_t s) {
  if (len <= 0) return;
  const bool vec = aligned16(W) && aligned16(T1) && aligned16(ACC) && (first || aligned16(T2)) &&
                   (last || aligned16(Tout));
  if (vec) {
    const int64_t np = len / 2, tail = (len & 1) ? len - 1 : -1;
    launch_cheb_series<d2v>(stream_grid(np, kChebPerCu), np, tail, W, T1, T2, alpha, beta, mu, mu0,
                            Tout, ACC, first, last, s);
    return;
  }
  launch_cheb_series<double>(stream_grid(len, kChebPerCu), len, (int64_t)-1, W, T1, T2, alpha, beta,
                             mu, mu0, Tout, ACC, first, last, s);
}

int moment_grid(int64_t nrows, int b) {
  return stream_grid(nrows * ((b + 1) / 2), kChebPerCu);
}

void cheb_moment_term(int64_t nrows, int b, const double* W, const double* T1, const double* T2,
                      double alpha, double beta, double* Tout, double* part, int grid, bool first,
                      bool last, hipStream_t s) {
  if (nrows <= 0 || b <= 0) return;
  // a thread keeps a column pair only when every row starts on a pair: b even
  const bool vec = b % 2 == 0 && aligned16(W) && aligned16(T1) && (first || aligned16(T2)) &&
                   (last || aligned16(Tout));
  if (vec)
    launch_cheb_moment<d2v>(grid, nrows, b / 2, W, T1, T2, alpha, beta, Tout, part, first, last, s);
  else
    launch_cheb_moment<double>(grid, nrows, b, W, T1, T2, alpha, beta, Tout, part, first, last, s);
}

void cheb_diag_term(int64_t nrows, int b, int nf, const double* W, const double* T1, const double* T2,
                    const double* X, double alpha, double beta, double* Tout, const double* coef,
                    double* D, double* qout, bool first, bool last, hipStream_t s) {
  if (nrows <= 0 || b <= 0 || b > kChebThreads || nf <= 0) return;
  const bool vec = b % 2 == 0 && aligned16(W) && aligned16(X) && (first || (aligned16(T1) && aligned16(T2))) &&
                   (last || aligned16(Tout));
  const int cw = vec ? b / 2 : b;
  const int nrg = kChebThreads / cw;
  const int64_t ntiles = (nrows + nrg - 1) / nrg;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)cu_count() * kChebPerCu));
  if (vec)
    launch_cheb_diag<d2v>(grid, nrows, cw, nf, W, T1, T2, X, alpha, beta, Tout, coef, D, qout, first, last, s);
  else
    launch_cheb_diag<double>(grid, nrows, cw, nf, W, T1, T2, X, alpha, beta, Tout, coef, D, qout, first, last,
                             s);
}

void sign_block(int64_t len, double* x, hipStream_t s) {
  if (len <= 0) return;
  hipLaunchKernelGGL(k_sign_block, dim3(stream_grid(len, kChebPerCu)), dim3(kChebThreads), 0, s, len, x);
}

int resid_grid(int64_t nrows) {
  const int64_t by_rows = (nrows + kResidMinRows - 1) / kResidMinRows;
  return (int)std::max<int64_t>(1, std::min<int64_t>(by_rows, (int64_t)cu_count() * kResidPerCu));
}

void resid_partial(int64_t nrows, int kp, const double* Z, const double* X, const double* theta,
                   double* part, int grid, hipStream_t s) {
  int cw = 1;
  while (cw < kp && cw < kChebThreads) cw *= 2;
  hipLaunchKernelGGL(k_resid_partial, dim3(grid), dim3(kChebThreads), 0, s, nrows, kp, cw, Z, X, theta,
                     part);
}

void copy_cols(int64_t nrows, int w, const double* src, int lds, int s0, double* dst, int ldd, int d0,
               hipStream_t s) {
  if (nrows <= 0 || w <= 0) return;
  const int grid = stream_grid(nrows * w, kChebPerCu);
  hipLaunchKernelGGL(k_copy_cols, dim3(grid), dim3(kChebThreads), 0, s, nrows, w, src, lds, s0, dst, ldd,
                     d0);
}

}  // namespace rbl
