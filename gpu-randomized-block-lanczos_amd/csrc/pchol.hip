// pchol.hip — partial pivoted Cholesky of the implicit kernel matrix (rbl_kernel_pchol):
//
//     L L^T ~ A = diag(s) K diag(s),    K_ij = kappa(x_i, x_j)    (the operator without its nugget),
//
// from the n x d points alone: R greedy steps, each one column of A (O(n d)) and one update against the
// earlier columns of L (O(n j)); A is never formed.
//
// State on the device: the residual diagonal d (n), L column-major n x R (zeroed at the start), the
// workgroups' partial records (d_max, index, trace) in two buffers, and the small records piv, trace,
// floor, rank and one stop flag per launch.
//
// k_pchol_init: d_i = s_i^2 kappa(x_i, x_i) by the operator's diagonal rule (kern_value, same = true, on
// nrm_i for the inner product), and each workgroup's partial into buffer 0.
//
// k_pchol_step, launch j = 0 .. R (R + 1 launches enqueued back to back, no host read in between):
//   * every workgroup reduces all partials of buffer j & 1 — thread t takes the slabs t, t + 256, ... in
//     ascending order, then a fixed LDS tree — so all arrive at the same pivot p (the largest d, the
//     smaller index on a tie; a NaN never wins), the same trace_j and the same stop decision without
//     talking to each other;
//   * stop (rank = j) when j == R, !(d_p > floor) with floor = 4 (R + 2) u dmax0, or trace_j <= tol
//     trace_0.  Workgroup 0 records trace[j] and either piv[j] or the rank and flag[j + 1]; a launch that
//     finds flag[j] set passes it on and returns.  flag[j] is written by launch j - 1 alone and read by
//     launch j alone: no word is written and read inside one launch;
//   * otherwise x_p and L[p, 0..j) go to LDS (wave-uniform reads from there on) and the thread that owns
//     row i forms
//         L[i, j] = (s_i s_p kappa(x_i, x_p) - sum_{l<j} L[i, l] L[p, l]) / sqrt(d_p),   l ascending,
//     sqrt(d_p) for i == p and exactly 0 where d_i == 0 before the step, then d_i <- max(d_i - L[i, j]^2,
//     0) (one fused multiply-add), d_p <- 0.  The earlier columns are read coalesced (column-major L, a
//     thread per row), x_i by 32-byte loads;
//   * each workgroup writes its partial (max d, index, sum d by a fixed LDS tree) to buffer (j + 1) & 1.
//     Two buffers because a workgroup of launch j that finishes early would otherwise overwrite a partial
//     a slower workgroup of the same launch has yet to read; launch j + 1 starts after launch j ended
//     (one stream), so the buffer it overwrites has no reader left.
//
// The grid is G = ceil(n / 256) slabs of 256 rows, a function of n alone: the bits do not depend on the
// device.  Every workgroup reading all G partials costs 20 G^2 bytes per step from cache: nothing up to
// n ~ 10^6 (G = 4096), more than the step's own traffic from n ~ 4 10^6 — a second reduction level would
// be the remedy there.  No atomics, no cooperative launch, no grid barrier, no waiting on device flags.
#include <algorithm>
#include <climits>
#include <cmath>

#include "kernelop_dev.hpp"
#include "kernels.hpp"

namespace rbl {

namespace {

using namespace kerndev;

constexpr int kT = kPcholSlabRows;  // rows per slab = threads per workgroup

// the order of the pivot search: the larger d, the smaller index on equal d
__device__ __forceinline__ bool pchol_better(double da, int32_t ia, double db, int32_t ib) {
  return da > db || (da == db && ia < ib);
}

// (d, i) <- the best of the workgroup's candidates, t <- their sum by a fixed tree; every thread gets
// the result.  The scratch may be reused after the return.
__device__ __forceinline__ void pchol_block_reduce(double& d, int32_t& i, double& t, double* sd, int32_t* si,
                                                   double* st) {
  const int tid = threadIdx.x;
  sd[tid] = d, si[tid] = i, st[tid] = t;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      if (pchol_better(sd[tid + s], si[tid + s], sd[tid], si[tid])) sd[tid] = sd[tid + s], si[tid] = si[tid + s];
      st[tid] += st[tid + s];
    }
    __syncthreads();
  }
  d = sd[0], i = si[0], t = st[0];
  __syncthreads();
}

template <int KIND>
__global__ __launch_bounds__(kT) void k_pchol_init(KernOp op, PcholWork W) {
  __shared__ double sd[kT], st[kT];
  __shared__ int32_t si[kT];
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  double d = -INFINITY, t = 0.0;
  int32_t idx = INT_MAX;
  if (i < op.n) {
    const double s = op.scale ? op.scale[i] : 1.0;
    const double ni = op.nrm[i];
    const double v = (s * s) * kern_value<KIND>(op.gamma, op.coef0, op.degree, ni, ni, ni, true);
    W.d[i] = v;
    t = v;
    idx = (int32_t)i;
    d = v == v ? v : -INFINITY;
  }
  pchol_block_reduce(d, idx, t, sd, si, st);
  if (threadIdx.x == 0) W.pmax[blockIdx.x] = d, W.pidx[blockIdx.x] = idx, W.ptrace[blockIdx.x] = t;
}

template <int KIND>
__global__ __launch_bounds__(kT) void k_pchol_step(KernOp op, PcholWork W, int j, int R, double tol) {
  __shared__ double sd[kT], st[kT], xp[kKernMaxDim], lp[kPcholMaxRank];
  __shared__ int32_t si[kT];
  const int tid = threadIdx.x;
  if (W.flag[j]) {  // stopped at an earlier launch
    if (blockIdx.x == 0 && tid == 0) W.flag[j + 1] = 1;
    return;
  }
  const int G = (int)gridDim.x;
  const int64_t n = op.n;
  // all partials of the launch before: the same pivot, trace and decision in every workgroup
  double dp = -INFINITY, tr = 0.0;
  int32_t pi = INT_MAX;
  {
    const double* pm = W.pmax + (size_t)(j & 1) * G;
    const double* pt = W.ptrace + (size_t)(j & 1) * G;
    const int32_t* px = W.pidx + (size_t)(j & 1) * G;
    for (int g = tid; g < G; g += kT) {
      const double dg = pm[g];
      const int32_t ig = px[g];
      if (pchol_better(dg, ig, dp, pi)) dp = dg, pi = ig;
      tr += pt[g];
    }
  }
  pchol_block_reduce(dp, pi, tr, sd, si, st);
  const double floor_ = j == 0 ? (double)(4 * (R + 2)) * 0x1p-53 * dp : W.floor_[0];
  const double tr0 = j == 0 ? tr : W.trace[0];
  const bool stop = j == R || !(dp > floor_) || tr <= tol * tr0;
  if (blockIdx.x == 0 && tid == 0) {
    W.trace[j] = tr;
    if (j == 0) W.floor_[0] = floor_;
    if (stop)
      W.rank[0] = j, W.flag[j + 1] = 1;
    else
      W.piv[j] = pi;
  }
  if (stop) return;
  // here d_p > floor >= 0: p is a row of the matrix
  const int64_t p = __builtin_amdgcn_readfirstlane(pi);
  const int d4 = op.d4;
  for (int k = tid; k < d4; k += kT) xp[k] = op.X[p * d4 + k];
  if (tid < j) lp[tid] = W.L[p + (int64_t)tid * W.ldl];
  __syncthreads();
  const double sq = sqrt(dp);
  const double sp = op.scale ? op.scale[p] : 1.0;
  const double np = op.nrm[p];

  const int64_t i = (int64_t)blockIdx.x * kT + tid;
  double dn = -INFINITY, t = 0.0;
  int32_t idx = INT_MAX;
  if (i < n) {
    const double di = W.d[i];
    double v = 0.0, dnew = 0.0;
    if (i == p) {
      v = sq;
    } else if (di != 0.0) {
      const d4v* xi = reinterpret_cast<const d4v*>(op.X + i * d4);
      double ip = 0.0;
      for (int k4 = 0; k4 < d4 / 4; ++k4) {
        const d4v x = xi[k4];
        ip = fma(xp[4 * k4 + 0], x.x, ip);
        ip = fma(xp[4 * k4 + 1], x.y, ip);
        ip = fma(xp[4 * k4 + 2], x.z, ip);
        ip = fma(xp[4 * k4 + 3], x.w, ip);
      }
      const double si_ = op.scale ? op.scale[i] : 1.0;
      const double a = (si_ * sp) * kern_value<KIND>(op.gamma, op.coef0, op.degree, op.nrm[i], np, ip, false);
      const double* Li = W.L + i;
      double sum = 0.0;
#pragma unroll 8
      for (int l = 0; l < j; ++l) sum = fma(Li[(int64_t)l * W.ldl], lp[l], sum);
      v = (a - sum) / sq;
      dnew = fmax(fma(-v, v, di), 0.0);
    }
    W.L[i + (int64_t)j * W.ldl] = v;
    W.d[i] = dnew;
    dn = dnew, t = dnew, idx = (int32_t)i;
  }
  pchol_block_reduce(dn, idx, t, sd, si, st);
  if (tid == 0) {
    const size_t o = (size_t)((j + 1) & 1) * G + blockIdx.x;
    W.pmax[o] = dn, W.pidx[o] = idx, W.ptrace[o] = t;
  }
}

template <int KIND>
void pchol_launch(const KernOp& op, int R, double tol, const PcholWork& W, hipStream_t s) {
  const unsigned grid = (unsigned)pchol_slabs(op.n);
  hipLaunchKernelGGL((k_pchol_init<KIND>), dim3(grid), dim3(kT), 0, s, op, W);
  for (int j = 0; j <= R; ++j) hipLaunchKernelGGL((k_pchol_step<KIND>), dim3(grid), dim3(kT), 0, s, op, W, j, R, tol);
}

}  // namespace

int pchol_slabs(int64_t n) { return (int)ceil_div(n, (int64_t)kPcholSlabRows); }

bool kernop_pchol(const KernOp& op, int R, double tol, const PcholWork& W, hipStream_t s) {
  if (op.n <= 0 || op.n > (int64_t)INT32_MAX - 64 || op.d4 < 4 || op.d4 > kKernMaxDim || (op.d4 & 3) || !op.X ||
      !op.nrm || R < 1 || R > kPcholMaxRank || R > op.n || !(tol >= 0.0 && tol < 1.0) || W.ldl < op.n || !W.L ||
      !W.d || !W.pmax || !W.ptrace || !W.pidx || !W.piv || !W.trace || !W.floor_ || !W.rank || !W.flag)
    return false;
  // L zero (columns past the rank stay so), piv -1, the flags clear
  if (hipMemsetAsync(W.L, 0, (size_t)W.ldl * R * sizeof(double), s) != hipSuccess ||
      hipMemsetAsync(W.piv, 0xff, (size_t)R * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(W.trace, 0, (size_t)(R + 1) * sizeof(double), s) != hipSuccess ||
      hipMemsetAsync(W.flag, 0, (size_t)(R + 2) * sizeof(int32_t), s) != hipSuccess)
    return false;
  if (op.kind == kKernRbf)
    pchol_launch<kKernRbf>(op, R, tol, W, s);
  else if (op.kind == kKernLaplace)
    pchol_launch<kKernLaplace>(op, R, tol, W, s);
  else if (op.kind == kKernPoly)
    pchol_launch<kKernPoly>(op, R, tol, W, s);
  else
    return false;
  return true;
}

}  // namespace rbl
