// cg.hip — the row passes of the batched preconditioned conjugate-gradient solver (gfx950).
//
// rbl_solve solves (Op + sigma I) X = B for b right-hand sides at once (rbl_api.cpp): every column
// runs its own Hestenes-Stiefel recurrence, all of them share one product W = Op P per iteration
// (apply_A, whatever the operator is), and the per-column scalars — rho, alpha, beta, |b|^2, |r|^2,
// the iteration count and the status — live in a small device array (CgScalars), so an iteration
// is a fixed sequence of launches with no host round trip:
//
//     W = Op P                                             apply_A
//     pap_c = p_c^T w_c + sigma p_c^T p_c                  k_cg_dot + reduce_slab   16 B / element
//     alpha_c = rho_c / pap_c                              k_cg_scalars (one workgroup)
//     x += alpha p,  r -= alpha (w + sigma p),  |r|^2      k_cg_update + reduce_slab   48 B
//     [w = V^T r,  c = dv o w]                             lr_project, k_cg_small (preconditioner)
//     rho' = r^T z,  beta = rho' / rho,  freeze            k_cg_scalars2 (one workgroup)
//     p = z + beta p,  z = r [+ V c]                       k_cg_dir   24 B (+ one read of V)
//
// The preconditioner is M^-1 = I + V diag(dv) V^T with V n x r orthonormal (r <= 32): z = r + V c
// is never stored — rho' = r^T r + w^T c comes from the small quantities and k_cg_dir adds V c with
// c in registers, as lr_update does (lowrank.hip; V is stored like its P: row-major, rows padded
// with zeros to rp = lr_padded_width(r)).
//
// A column is frozen once |r|^2 <= tol^2 |b|^2 (status 0), or when p^T (Op + sigma) p is <= 0 or
// not finite (status 2): from then on its x, r and p are never stored again (a thread that holds a
// column pair of which one is frozen stores that column's old bits), so the result does not depend
// on how many further iterations the other columns, or the host's check interval, let run.
//
// Every column sum uses the scheme of k_cheb_moment (spmm_cheb.hip): a row is cw slots of type T
// (d2v: b / 2 column pairs and 16-byte accesses for even b; double: b columns), a thread keeps its
// slot for the whole pass, the workgroup covers a tile of nrg = 256 / cw rows at a time and walks
// the tiles grid-stride (grid from the CU count), a row wider than 256 slots runs in chunks of
// 256.  Each thread sums its rows ascending, the row groups are added ascending in LDS, and
// reduce_slab adds the workgroups in order: no atomics, two runs give the same bits.
#include <algorithm>
#include <atomic>

#include "kernels.hpp"

namespace rbl {

namespace {

constexpr int kCgThreads = 256;
constexpr int kCgPerCu = 8;  // workgroups per CU (2 waves per SIMD x 4), as the other stream passes

int cg_cu_count() {
  static std::atomic<int> cus[64];  // per device; zero-initialised (static storage)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cus[dev].load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
      v = 256;
    cus[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

// A thread's slot of the per-column scalars: one column (double) or a column pair (d2v).
template <typename T>
struct Col;
template <>
struct Col<double> {
  static __device__ __forceinline__ double load(const double* a, int c) { return a[c]; }
  static __device__ __forceinline__ int active(const int* st, int c) { return st[c] == kCgActive ? 1 : 0; }
  static __device__ __forceinline__ double pick(int m, double nv, double ov) { return m ? nv : ov; }
  static __device__ __forceinline__ double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
  static __device__ __forceinline__ void stage(double* sm, int q, double v) {
    sm[q * kCgThreads + threadIdx.x] = v;
  }
};
template <>
struct Col<d2v> {
  static __device__ __forceinline__ d2v load(const double* a, int c) {
    d2v v;
    v.x = a[2 * c];
    v.y = a[2 * c + 1];
    return v;
  }
  static __device__ __forceinline__ int active(const int* st, int c) {
    return (st[2 * c] == kCgActive ? 1 : 0) | (st[2 * c + 1] == kCgActive ? 2 : 0);
  }
  static __device__ __forceinline__ d2v pick(int m, d2v nv, d2v ov) {
    d2v v;
    v.x = (m & 1) ? nv.x : ov.x;
    v.y = (m & 2) ? nv.y : ov.y;
    return v;
  }
  static __device__ __forceinline__ d2v fma(d2v a, d2v b, d2v c) {
    d2v v;
    v.x = __builtin_fma(a.x, b.x, c.x);
    v.y = __builtin_fma(a.y, b.y, c.y);
    return v;
  }
  static __device__ __forceinline__ void stage(double* sm, int q, d2v v) {
    sm[(2 * q) * kCgThreads + threadIdx.x] = v.x;
    sm[(2 * q + 1) * kCgThreads + threadIdx.x] = v.y;
  }
};

// The workgroup's NQ column sums of one chunk of slots: the threads' sums staged in LDS, then one
// thread per (quantity, column) adds the row groups ascending and writes out[q][column] (out: NQ x b).
template <typename T, int NQ>
__device__ __forceinline__ void cg_col_sums(double* sm, const T (&acc)[NQ], double* out, int cb, int cw,
                                            int cwl, int nrg) {
  constexpr int VW = sizeof(T) / sizeof(double);
#pragma unroll
  for (int q = 0; q < NQ; ++q) Col<T>::stage(sm, q, acc[q]);
  __syncthreads();
  const int ncl = cw - cb < cwl ? cw - cb : cwl;  // slots of this chunk
  for (int idx = threadIdx.x; idx < NQ * VW * ncl; idx += kCgThreads) {
    const int qv = idx / ncl, c2 = idx % ncl;  // qv = q * VW + lane of the slot
    double s = 0.0;
    for (int g = 0; g < nrg; ++g) s += sm[qv * kCgThreads + g * cwl + c2];
    out[(qv / VW) * (VW * cw) + (cb + c2) * VW + qv % VW] = s;
  }
  __syncthreads();
}

// R = B - (W + sigma X) (HAS_X; else R = B) and the partials of |b|^2 and |r|^2 per column:
// part[g][0][c], part[g][1][c].  The first residual of a run and the true residual at its end.
template <typename T, bool HAS_X>
__global__ __launch_bounds__(kCgThreads) void k_cg_resid(int64_t nrows, int cw, const T* __restrict__ B,
                                                         const T* __restrict__ W,
                                                         const T* __restrict__ X, double sigma,
                                                         T* __restrict__ R, double* __restrict__ part) {
  constexpr int VW = sizeof(T) / sizeof(double);
  __shared__ double sm[2 * VW * kCgThreads];
  const int cwl = cw < kCgThreads ? cw : kCgThreads;
  const int nrg = kCgThreads / cwl;
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  double* out = part + (int64_t)blockIdx.x * 2 * VW * cw;
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    T acc[2] = {T(0.0), T(0.0)};
    if (rg < nrg && c < cw) {
      for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < nrows; r += rstride) {
        const int64_t i = r * cw + c;
        const T bv = B[i];
        T rv = bv;
        if constexpr (HAS_X) rv = bv - (W[i] + sigma * X[i]);
        R[i] = rv;
        acc[0] += bv * bv;
        acc[1] += rv * rv;
      }
    }
    cg_col_sums<T, 2>(sm, acc, out, cb, cw, cwl, nrg);
  }
}

// part[g][c] = workgroup g's share of p_c^T (w_c + sigma p_c)
template <typename T>
__global__ __launch_bounds__(kCgThreads) void k_cg_dot(int64_t nrows, int cw, const T* __restrict__ P,
                                                       const T* __restrict__ W, double sigma,
                                                       double* __restrict__ part) {
  constexpr int VW = sizeof(T) / sizeof(double);
  __shared__ double sm[VW * kCgThreads];
  const int cwl = cw < kCgThreads ? cw : kCgThreads;
  const int nrg = kCgThreads / cwl;
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  double* out = part + (int64_t)blockIdx.x * VW * cw;
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    T acc[1] = {T(0.0)};
    if (rg < nrg && c < cw) {
      for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < nrows; r += rstride) {
        const int64_t i = r * cw + c;
        const T p = P[i];
        acc[0] += p * (W[i] + sigma * p);
      }
    }
    cg_col_sums<T, 1>(sm, acc, out, cb, cw, cwl, nrg);
  }
}

// x += alpha p, r -= alpha (w + sigma p) for the active columns, and part[g][c] = the share of
// |r_c|^2 after the update.  A slot whose columns are all frozen is neither read nor written; the
// sums of frozen columns are not used.
template <typename T>
__global__ __launch_bounds__(kCgThreads) void k_cg_update(int64_t nrows, int cw, T* __restrict__ X,
                                                          T* __restrict__ R, const T* __restrict__ P,
                                                          const T* __restrict__ W, double sigma,
                                                          const double* __restrict__ alpha,
                                                          const int* __restrict__ status,
                                                          double* __restrict__ part) {
  constexpr int VW = sizeof(T) / sizeof(double);
  __shared__ double sm[VW * kCgThreads];
  const int cwl = cw < kCgThreads ? cw : kCgThreads;
  const int nrg = kCgThreads / cwl;
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  double* out = part + (int64_t)blockIdx.x * VW * cw;
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    T acc[1] = {T(0.0)};
    if (rg < nrg && c < cw) {
      const int m = Col<T>::active(status, c);
      if (m) {
        const T a = Col<T>::load(alpha, c);
        for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < nrows; r += rstride) {
          const int64_t i = r * cw + c;
          const T p = P[i], x = X[i], rv = R[i];
          const T q = W[i] + sigma * p;
          const T rn = Col<T>::pick(m, Col<T>::fma(-a, q, rv), rv);
          X[i] = Col<T>::pick(m, Col<T>::fma(a, p, x), x);
          R[i] = rn;
          acc[0] += rn * rn;
        }
      }
    }
    cg_col_sums<T, 1>(sm, acc, out, cb, cw, cwl, nrg);
  }
}

// p = z + beta p for the active columns, z = r (RP = 0) or r + V c (V: rows of RP doubles, c: RP x b
// row-major with the slot's RP entries in registers).
template <typename T, int RP>
__global__ __launch_bounds__(kCgThreads) void k_cg_dir(int64_t nrows, int cw, const T* __restrict__ R,
                                                       T* __restrict__ P, const double* __restrict__ V,
                                                       const T* __restrict__ C,
                                                       const double* __restrict__ beta,
                                                       const int* __restrict__ status) {
  const int cwl = cw < kCgThreads ? cw : kCgThreads;
  const int nrg = kCgThreads / cwl;
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  if (rg >= nrg) return;
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    if (c >= cw) continue;
    const int m = Col<T>::active(status, c);
    if (!m) continue;
    const T bt = Col<T>::load(beta, c);
    T cj[RP > 0 ? RP : 1];
    if constexpr (RP > 0) {
#pragma unroll
      for (int j = 0; j < RP; ++j) cj[j] = C[(int64_t)j * cw + c];
    }
    for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < nrows; r += rstride) {
      const int64_t i = r * cw + c;
      T z = R[i];
      const T p = P[i];
      if constexpr (RP > 0) {
        const d2v* v = reinterpret_cast<const d2v*>(V + r * RP);
        T t = T(0.0);
#pragma unroll
        for (int j = 0; j < RP; j += 2) {
          const d2v vj = v[j / 2];
          t += vj.x * cj[j];
          t += vj.y * cj[j + 1];
        }
        z = z + t;
      }
      P[i] = Col<T>::pick(m, Col<T>::fma(bt, p, z), p);
    }
  }
}

// c = diag(dv) w: w and c rp x b row-major, dv rp entries (zero past r)
__global__ __launch_bounds__(kCgThreads) void k_cg_small(int rp, int b, const double* __restrict__ dv,
                                                         const double* __restrict__ w,
                                                         double* __restrict__ c) {
  for (int idx = threadIdx.x; idx < rp * b; idx += kCgThreads) c[idx] = dv[idx / b] * w[idx];
}

__device__ __forceinline__ bool cg_pos_finite(double v) { return v > 0.0 && v < __builtin_inf(); }

// alpha_c = rho_c / pap_c; a frozen column gets 0; pap_c <= 0 or not finite freezes the column as
// not positive definite
__global__ __launch_bounds__(kCgThreads) void k_cg_scalars(int b, const double* __restrict__ pap,
                                                           CgScalars s) {
  for (int c = threadIdx.x; c < b; c += kCgThreads) {
    double a = 0.0;
    if (s.status[c] == kCgActive) {
      const double den = pap[c];
      if (cg_pos_finite(den)) a = s.rho[c] / den;
      else s.status[c] = kCgNotPosDef;
    }
    s.alpha[c] = a;
  }
}

// After the residual update (or, init, after the first residual: dots = [|b|^2, |r|^2]):
// rho' = |r|^2 + w^T c (rp > 0), beta = rho' / rho, the iteration counted and (alpha, beta) appended
// to the history, the column frozen once |r|^2 <= tol^2 |b|^2, and the active columns counted.
__global__ __launch_bounds__(kCgThreads) void k_cg_scalars2(int b, int rp, int init, int iter,
                                                            const double* __restrict__ dots,
                                                            const double* __restrict__ w,
                                                            const double* __restrict__ cc, double tol2,
                                                            CgScalars s) {
  __shared__ int cnt[kCgThreads];
  int mine = 0;
  for (int c = threadIdx.x; c < b; c += kCgThreads) {
    double bb, rr;
    if (init) {
      bb = dots[c];
      rr = dots[b + c];
      s.bb[c] = bb;
      s.iters[c] = 0;
      s.alpha[c] = 0.0;
    } else {
      if (s.status[c] != kCgActive) {
        s.beta[c] = 0.0;
        continue;
      }
      bb = s.bb[c];
      rr = dots[c];
    }
    s.rr[c] = rr;
    double rho = rr;
    for (int j = 0; j < rp; ++j) rho += w[j * b + c] * cc[j * b + c];
    double bt = 0.0;
    if (!init) {
      bt = rho / s.rho[c];
      s.iters[c] += 1;
      if (s.hist) {
        s.hist[((int64_t)2 * iter) * b + c] = s.alpha[c];
        s.hist[((int64_t)2 * iter + 1) * b + c] = bt;
      }
    }
    int st = kCgActive;
    if (rr <= tol2 * bb) st = kCgConverged;
    else if (!cg_pos_finite(rho) || !cg_pos_finite(rr)) st = kCgNotPosDef;
    s.rho[c] = rho;
    s.beta[c] = bt;
    s.status[c] = st;
    mine += st == kCgActive ? 1 : 0;
  }
  cnt[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int t = 0; t < kCgThreads; ++t) total += cnt[t];
    *s.nactive = total;
  }
}

bool cg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
const T* as(const double* p) { return reinterpret_cast<const T*>(p); }
template <typename T>
T* as(double* p) { return reinterpret_cast<T*>(p); }

}  // namespace

int cg_grid(int64_t nrows, int b) {
  const int64_t want = (nrows * ((b + 1) / 2) + kCgThreads - 1) / kCgThreads;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cg_cu_count() * kCgPerCu));
}

void cg_resid(int64_t nrows, int b, const double* B, const double* W, const double* X, double sigma,
              double* R, double* part, double* dots, hipStream_t s) {
  if (nrows <= 0 || b < 1) return;
  const int grid = cg_grid(nrows, b);
  const bool vec = b % 2 == 0 && cg_aligned16(B) && cg_aligned16(R) && (!X || (cg_aligned16(W) && cg_aligned16(X)));
#define RBL_CG_RESID(T, HX, CW)                                                                      \
  hipLaunchKernelGGL((k_cg_resid<T, HX>), dim3(grid), dim3(kCgThreads), 0, s, nrows, CW, as<T>(B),   \
                     as<T>(W), as<T>(X), sigma, as<T>(R), part)
  if (vec) {
    if (X) RBL_CG_RESID(d2v, true, b / 2);
    else RBL_CG_RESID(d2v, false, b / 2);
  } else {
    if (X) RBL_CG_RESID(double, true, b);
    else RBL_CG_RESID(double, false, b);
  }
#undef RBL_CG_RESID
  reduce_slab(part, grid, (int64_t)2 * b, dots, nullptr, s);
}

void cg_dot(int64_t nrows, int b, const double* P, const double* W, double sigma, double* part,
            double* dots, hipStream_t s) {
  if (nrows <= 0 || b < 1) return;
  const int grid = cg_grid(nrows, b);
  if (b % 2 == 0 && cg_aligned16(P) && cg_aligned16(W))
    hipLaunchKernelGGL((k_cg_dot<d2v>), dim3(grid), dim3(kCgThreads), 0, s, nrows, b / 2, as<d2v>(P),
                       as<d2v>(W), sigma, part);
  else
    hipLaunchKernelGGL((k_cg_dot<double>), dim3(grid), dim3(kCgThreads), 0, s, nrows, b, P, W, sigma, part);
  reduce_slab(part, grid, (int64_t)b, dots, nullptr, s);
}

void cg_alpha(int b, const double* pap, const CgScalars& sc, hipStream_t s) {
  hipLaunchKernelGGL(k_cg_scalars, dim3(1), dim3(kCgThreads), 0, s, b, pap, sc);
}

void cg_update(int64_t nrows, int b, double* X, double* R, const double* P, const double* W, double sigma,
               const CgScalars& sc, double* part, double* dots, hipStream_t s) {
  if (nrows <= 0 || b < 1) return;
  const int grid = cg_grid(nrows, b);
  if (b % 2 == 0 && cg_aligned16(X) && cg_aligned16(R) && cg_aligned16(P) && cg_aligned16(W))
    hipLaunchKernelGGL((k_cg_update<d2v>), dim3(grid), dim3(kCgThreads), 0, s, nrows, b / 2, as<d2v>(X),
                       as<d2v>(R), as<d2v>(P), as<d2v>(W), sigma, sc.alpha, sc.status, part);
  else
    hipLaunchKernelGGL((k_cg_update<double>), dim3(grid), dim3(kCgThreads), 0, s, nrows, b, X, R, P, W,
                       sigma, sc.alpha, sc.status, part);
  reduce_slab(part, grid, (int64_t)b, dots, nullptr, s);
}

void cg_small(int rp, int b, const double* dv, const double* w, double* c, hipStream_t s) {
  if (rp < 1 || b < 1) return;
  hipLaunchKernelGGL(k_cg_small, dim3(1), dim3(kCgThreads), 0, s, rp, b, dv, w, c);
}

void cg_beta(int b, int rp, bool init, int iter, const double* dots, const double* w, const double* c,
             double tol2, const CgScalars& sc, hipStream_t s) {
  hipLaunchKernelGGL(k_cg_scalars2, dim3(1), dim3(kCgThreads), 0, s, b, rp, init ? 1 : 0, iter, dots, w, c,
                     tol2, sc);
}

void cg_dir(int64_t nrows, int b, int rp, const double* R, double* P, const double* V, const double* c,
            const CgScalars& sc, hipStream_t s) {
  if (nrows <= 0 || b < 1 || (rp != 0 && rp != lr_padded_width(rp))) return;
  const int grid = cg_grid(nrows, b);
  const bool vec = b % 2 == 0 && cg_aligned16(R) && cg_aligned16(P) && (rp == 0 || cg_aligned16(c));
#define RBL_CG_DIR(RP)                                                                                \
  do {                                                                                                \
    if (vec)                                                                                          \
      hipLaunchKernelGGL((k_cg_dir<d2v, RP>), dim3(grid), dim3(kCgThreads), 0, s, nrows, b / 2,       \
                         as<d2v>(R), as<d2v>(P), V, as<d2v>(c), sc.beta, sc.status);                  \
    else                                                                                              \
      hipLaunchKernelGGL((k_cg_dir<double, RP>), dim3(grid), dim3(kCgThreads), 0, s, nrows, b, R, P, V, \
                         c, sc.beta, sc.status);                                                      \
  } while (0)
  switch (rp) {
    case 0: RBL_CG_DIR(0); break;
    case 2: RBL_CG_DIR(2); break;
    case 4: RBL_CG_DIR(4); break;
    case 6: RBL_CG_DIR(6); break;
    case 8: RBL_CG_DIR(8); break;
    case 12: RBL_CG_DIR(12); break;
    case 16: RBL_CG_DIR(16); break;
    case 24: RBL_CG_DIR(24); break;
    case 32: RBL_CG_DIR(32); break;
    default: break;
  }
#undef RBL_CG_DIR
}

}  // namespace rbl
