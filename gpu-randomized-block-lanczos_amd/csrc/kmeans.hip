// kmeans.hip — Lloyd's k-means over n points in d dimensions (rbl_kmeans_run) and k-means++ seeding
// (rbl_kmeans_seed), fp64, one GPU.  The points and the centres are held as the kernel matrix holds
// its points: row-major, zero-padded to d4 = 4 ceil(d / 4) columns, squared norms from kernop_norms.
//
// One Lloyd iteration is three launches and a reduction:
//
//   k_kmeans_assign   label_i = the j with the smallest (d2(i, j), j),
//                         d2(i, j) = max((|x_i|^2 + |c_j|^2) - 2 x_i.c_j, 0),
//                     the contract of kernelop_knn.hip with k = 1: the same pair tiles on
//                     v_mfma_f64_16x16x4_f64, the centres staged through LDS one stage ahead.  With
//                     k = 1 there is no list: a lane keeps its best (d2, j) in registers across the
//                     stages and the four lanes of a row combine once at the end, under the same
//                     order.  The column range (<= 256 centres) is not split; grid ceil(n / 64).
//                     Writes label_i and dmin_i = d2(i, label_i).
//   k_kmeans_update   per row slab g and cluster tile: sum_j, count_j, the inertia and the number of
//                     changed labels, as the partial record part[g][c d4 + c + 2].  A thread owns one
//                     column of one row lane and walks the lane's rows in ascending order, adding
//                     into the lane's c x d4 partial in LDS; one owner thread per output then adds
//                     the lanes' partials in ascending lane order.  No atomics.
//   reduce_slab       the slabs' records added in ascending slab order.
//   k_kmeans_form     centre_j = sum_j / (double)count_j (an IEEE division; a centre with count 0
//                     keeps its value), |C_new - C_old|_F^2 in a fixed order, and the decision record
//                     {inertia, changed, shift^2} the host reads once per iteration.
//
// Every summation order is a function of (n, d4, c) alone (kmeans_geometry), never of the device, so
// the bits do not depend on the CU count and two calls agree.
//
// Seeding round r >= 1: k_kmeans_assign against the one point picked last (its row of X is the centre
// array), then k_kmeans_seed_round — w_i = min(w_i, d2(i, last)), 0 by index for the point picked last
// (an earlier pick stays 0 under the min), and the total of every slab of 2048 points — and
// k_kmeans_seed_pick, one workgroup: the slab totals in 256 contiguous chunks, the total, and the walk
// chunks -> slabs of the chunk -> the 256 runs of 8 points of the slab -> the 8 points for the smallest
// i whose inclusive prefix sum exceeds u_r total.  Every level's order is a function of n alone.
#include <algorithm>
#include <climits>
#include <limits>

#include "kernelop_dev.hpp"
#include "kernels.hpp"

namespace rbl {

namespace {

using namespace kerndev;

// (d, j) before (td, tj): the order of the assignment
__device__ __forceinline__ bool km_before(double d, int j, double td, int tj) {
  return d < td || (d == td && j < tj);
}

// a stage buffer: C_j^T, the norms, and one spare double that takes the stores of the threads past the stage
constexpr int km_stage_doubles(int KS) { return 4 * KS * (kern_jt(KS) + 1) + kern_jt(KS) + 1; }
constexpr int km_assign_lds_bytes(int KS) { return 2 * km_stage_doubles(KS) * (int)sizeof(double); }

// X n x d4 with norms xn; C c x d4 with norms cn.  label (may be null) and dmin: n entries.
template <int KS>
__global__ __launch_bounds__(256) void k_kmeans_assign(int64_t n, int d4, int ks, int c,
                                                       const double* __restrict__ X,
                                                       const double* __restrict__ xn,
                                                       const double* __restrict__ C,
                                                       const double* __restrict__ cn,
                                                       int32_t* __restrict__ label, double* __restrict__ dmin) {
  constexpr int JT = kern_jt(KS);
  constexpr int LDX = JT + 1;            // C_j^T in LDS: element (k, j) at k LDX + j
  constexpr int XPER = JT * 4 * KS / 256;
  constexpr int BUF = km_stage_doubles(KS);
  extern __shared__ double km_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int64_t gi = (int64_t)blockIdx.x * 64 + 16 * wave + li;

  // the wave's X_i fragment and its norm
  double xi[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) xi[kk] = (kk < ks && gi < n) ? X[gi * d4 + 4 * kk + q] : 0.0;
  const double ni = gi < n ? xn[gi] : 0.0;

  // where this thread's staged elements of C go (the same every stage)
  const int xcount = JT * d4;
  const int ctot = c * d4;
  int xofs[XPER];
#pragma unroll
  for (int m = 0; m < XPER; ++m) {
    const int e = tid + 256 * m;
    xofs[m] = e < xcount ? (e % d4) * LDX + e / d4 : BUF - 1;   // (past the stage: the spare double)
  }
  double xr[XPER], nr = 0.0;
  auto load = [&](int j0) {
    const int lim = min(xcount, ctot - j0 * d4);   // this stage's elements that exist (wave-uniform)
#pragma unroll
    for (int m = 0; m < XPER; ++m) {
      const int e = tid + 256 * m;
      xr[m] = e < lim ? C[j0 * d4 + e] : 0.0;
    }
    if (tid < JT) nr = j0 + tid < c ? cn[j0 + tid] : 0.0;
  };
  auto store = [&](double* buf) {
#pragma unroll
    for (int m = 0; m < XPER; ++m) buf[xofs[m]] = xr[m];
    if (tid < JT) buf[4 * KS * LDX + tid] = nr;
  };

  const int nst = (c + JT - 1) / JT;
  if constexpr (KS >= 64) {  // the C rows past d4 of both buffers, which no stage writes: zero
    for (int e = tid; e < 2 * BUF; e += 256)
      if (e % BUF < 4 * KS * LDX) km_lds[e] = 0.0;
    __syncthreads();
  }
  double bd = std::numeric_limits<double>::infinity();
  int bj = INT_MAX;
  load(0);
  store(km_lds);
  __syncthreads();
  for (int s = 0; s < nst; ++s) {
    const int j0 = s * JT;
    if (s + 1 < nst) load(j0 + JT);
    const double* xs = km_lds + (s & 1) * BUF;
    const double* ns = xs + 4 * KS * LDX;
#pragma unroll
    for (int t = 0; t < JT / 16; ++t) {
      if (j0 + 16 * t >= c) break;  // a pair tile wholly past c has no candidate
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
        // groups of 4 steps under one guard each: the steps of the last group past ks multiply the
        // zeroed LDS rows by the zero tail of xi and add exact zeros
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
      // the four candidates of this lane: centres j0 + 16 t + q + 4 r of row gi
      const int jb = j0 + 16 * t + q;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jb + 4 * r;
        const double cd = fmax((ni + ns[16 * t + q + 4 * r]) - 2.0 * p[r], 0.0);
        if (j < c && km_before(cd, j, bd, bj)) bd = cd, bj = j;
      }
    }
    if (s + 1 < nst) store(km_lds + ((s + 1) & 1) * BUF);
    __syncthreads();
  }
  // the four lanes q of a row (li, li + 16, li + 32, li + 48) combine under the same order
#pragma unroll
  for (int m = 16; m <= 32; m <<= 1) {
    const double od = __shfl_xor(bd, m);
    const int oj = __shfl_xor(bj, m);
    if (km_before(od, oj, bd, bj)) bd = od, bj = oj;
  }
  if (q == 0 && gi < n) {
    if (label) label[gi] = bj;
    dmin[gi] = bd;
  }
}

template <int KS>
void launch_assign(int64_t n, int d4, int c, const double* X, const double* xn, const double* C, const double* cn,
                   int32_t* label, double* dmin, hipStream_t s) {
  constexpr int lds = km_assign_lds_bytes(KS);
  ensure_lds_attr(reinterpret_cast<const void*>(&k_kmeans_assign<KS>), lds);
  hipLaunchKernelGGL((k_kmeans_assign<KS>), dim3((unsigned)ceil_div(n, 64)), dim3(256), lds, s, n, d4, d4 / 4, c, X,
                     xn, C, cn, label, dmin);
}

// slab g = blockIdx.x covers rows [g rows_per, min(n, (g + 1) rows_per)), cluster tile blockIdx.y the
// centres [tile CW, min(c, (tile + 1) CW)).  Thread (rl, col) = (tid / d4, tid % d4), rl < RL.
__global__ __launch_bounds__(256) void k_kmeans_update(int64_t n, int d4, int c, int CW, int RL, int64_t rows_per,
                                                       const double* __restrict__ X,
                                                       const int32_t* __restrict__ label,
                                                       const int32_t* __restrict__ prev,
                                                       const double* __restrict__ dmin, double* __restrict__ part,
                                                       int64_t len) {
  extern __shared__ double km_lds[];
  const int tid = threadIdx.x;
  const int plane = CW * d4;               // one row lane's partial sums
  double* acc = km_lds;                    // RL x CW x d4
  double* iner = acc + RL * plane;         // RL
  int* cnt = reinterpret_cast<int*>(iner + RL);   // RL x CW
  int* chg = cnt + RL * CW;                // RL
  const int tile = blockIdx.y, c0 = tile * CW, cw = min(CW, c - c0);
  for (int e = tid; e < RL * plane; e += 256) acc[e] = 0.0;
  for (int e = tid; e < RL * CW; e += 256) cnt[e] = 0;
  if (tid < RL) iner[tid] = 0.0, chg[tid] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = min(n, r0 + rows_per);
  const int rl = tid / d4, col = tid - rl * d4;
  if (rl < RL) {
    const int64_t per = (rows_per + RL - 1) / RL;
    const int64_t a = r0 + rl * per, b = min(r1, a + per);
    double* my = acc + rl * plane + col;
    int* mycnt = cnt + rl * CW;
    const bool scal = col == 0 && tile == 0;
    double in = 0.0;
    int ch = 0;
    int64_t i = a;
    for (; i + 4 <= b; i += 4) {   // four rows' loads in flight, their additions in ascending row order
      int l[4];
      double x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) l[u] = label[i + u];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = (unsigned)(l[u] - c0) < (unsigned)cw ? X[(i + u) * d4 + col] : 0.0;
      if (scal) {
#pragma unroll
        for (int u = 0; u < 4; ++u) in += dmin[i + u], ch += l[u] != prev[i + u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = l[u] - c0;
        if ((unsigned)j < (unsigned)cw) {
          my[j * d4] += x[u];
          if (col == 0) ++mycnt[j];
        }
      }
    }
    for (; i < b; ++i) {
      const int l = label[i], j = l - c0;
      if (scal) in += dmin[i], ch += l != prev[i];
      if ((unsigned)j < (unsigned)cw) {
        my[j * d4] += X[i * d4 + col];
        if (col == 0) ++mycnt[j];
      }
    }
    if (scal) iner[rl] = in, chg[rl] = ch;
  }
  __syncthreads();
  // one owner thread per output: the row lanes' partials in ascending lane order
  double* out = part + (int64_t)blockIdx.x * len;
  for (int e = tid; e < cw * d4; e += 256) {
    double s = acc[e];
    for (int r = 1; r < RL; ++r) s += acc[r * plane + e];
    out[c0 * d4 + e] = s;
  }
  for (int e = tid; e < cw; e += 256) {
    int s = 0;
    for (int r = 0; r < RL; ++r) s += cnt[r * CW + e];
    out[(int64_t)c * d4 + c0 + e] = (double)s;
  }
  if (tile == 0 && tid == 0) {
    double s = iner[0];
    int k = chg[0];
    for (int r = 1; r < RL; ++r) s += iner[r], k += chg[r];
    out[(int64_t)c * d4 + c] = s;
    out[(int64_t)c * d4 + c + 1] = (double)k;
  }
}

// tot: the reduced record.  Cn = the new centres, rec = {inertia, changed, |Cn - Co|_F^2}: thread t adds
// its entries t, t + 256, ... in ascending order, thread 0 the 256 partials in ascending order.
__global__ __launch_bounds__(256) void k_kmeans_form(int c, int d4, const double* __restrict__ tot,
                                                     const double* __restrict__ Co, double* __restrict__ Cn,
                                                     double* __restrict__ rec) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int e = tid; e < c * d4; e += 256) {
    const double cntj = tot[c * d4 + e / d4], old = Co[e];
    const double v = cntj > 0.0 ? tot[e] / cntj : old;
    Cn[e] = v;
    const double df = v - old;
    s = fma(df, df, s);
  }
  sh[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double t = sh[0];
    for (int r = 1; r < 256; ++r) t += sh[r];
    rec[0] = tot[c * d4 + c];
    rec[1] = tot[c * d4 + c + 1];
    rec[2] = t;
  }
}

__global__ __launch_bounds__(256) void k_fill_i32(int64_t n, int32_t v, int32_t* __restrict__ p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- seeding ---------------------------------------------------------------------------------------
constexpr int kSeedRun = 8, kSeedSlab = 256 * kSeedRun;   // a thread's run of points; a slab of 2048

// w_i <- (i == last ? 0 : first ? dnew_i : min(w_i, dnew_i)); slabtot[s] = the slab's total: every
// thread its run of 8 in ascending order, thread 0 the 256 runs in ascending order
__global__ __launch_bounds__(256) void k_kmeans_seed_round(int64_t n, int first, int64_t last,
                                                           const double* __restrict__ dnew, double* __restrict__ w,
                                                           double* __restrict__ slabtot) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kSeedSlab + tid * kSeedRun;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < kSeedRun; ++e) {
    const int64_t i = i0 + e;
    if (i < n) {
      const double v = i == last ? 0.0 : first ? dnew[i] : fmin(w[i], dnew[i]);
      w[i] = v;
      s += v;
    }
  }
  sh[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double t = sh[0];
    for (int r = 1; r < 256; ++r) t += sh[r];
    slabtot[blockIdx.x] = t;
  }
}

// the first k < m with base + (v_0 + .. + v_k, added one at a time) > target; *base becomes the sum
// before v_k.  None (rounding at the upper end of u): the last k with v_k > 0, which exists whenever
// the level's total is positive.  over: an upper level already fell back, take the last positive.
template <class F>
__device__ int64_t km_walk(int64_t m, F v, double target, double* base, bool* over) {
  double run = *base, before_last = *base;
  int64_t last = -1;
  for (int64_t k = 0; k < m; ++k) {
    const double x = v(k);
    if (x > 0.0) last = k, before_last = run;
    const double nxt = run + x;
    if (!*over && nxt > target) {
      *base = run;
      return k;
    }
    run = nxt;
  }
  *over = true;
  *base = before_last;
  return last < 0 ? 0 : last;
}

// picked[r] <- the point of round r (the header of this file); one workgroup
__global__ __launch_bounds__(256) void k_kmeans_seed_pick(int64_t n, int64_t NS, const double* __restrict__ w,
                                                          const double* __restrict__ slabtot, double u, int r,
                                                          int32_t* __restrict__ picked) {
  __shared__ double sh[256];
  __shared__ double s_base, s_target;
  __shared__ int64_t s_slab;
  __shared__ int s_over;
  const int tid = threadIdx.x;
  const int64_t CH = (NS + 255) / 256;
  {
    const int64_t a = tid * CH, b = min(NS, a + CH);
    double s = 0.0;
    for (int64_t k = a; k < b; ++k) s += slabtot[k];
    sh[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double total = sh[0];
    for (int t = 1; t < 256; ++t) total += sh[t];
    s_slab = -1;
    if (!(total > 0.0)) {   // every point coincides with a picked one: the smallest index not picked
      int cand = 0;
      for (bool hit = true; hit;) {
        hit = false;
        for (int k = 0; k < r; ++k)
          if (picked[k] == cand) hit = true;
        if (hit) ++cand;
      }
      picked[r] = cand;
    } else {
      const double target = u * total;
      double base = 0.0;
      bool over = false;
      const int64_t kc = km_walk(256, [&](int64_t k) { return sh[k]; }, target, &base, &over);
      const int64_t a = kc * CH, b = min(NS, a + CH);
      const int64_t ksl = a + km_walk(b - a, [&](int64_t k) { return slabtot[a + k]; }, target, &base, &over);
      s_slab = ksl, s_base = base, s_target = target, s_over = over;
    }
  }
  __syncthreads();
  const int64_t slab = s_slab;
  if (slab < 0) return;
  const int64_t i0 = slab * kSeedSlab + tid * kSeedRun;
  {
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < kSeedRun; ++e)
      if (i0 + e < n) s += w[i0 + e];
    sh[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double base = s_base;
    bool over = s_over != 0;
    const int64_t kt = km_walk(256, [&](int64_t k) { return sh[k]; }, s_target, &base, &over);
    const int64_t j0 = slab * kSeedSlab + kt * kSeedRun;
    const int64_t m = min((int64_t)kSeedRun, n - j0);
    const int64_t ke = km_walk(m, [&](int64_t k) { return w[j0 + k]; }, s_target, &base, &over);
    picked[r] = (int32_t)(j0 + ke);
  }
}

bool km_shape_ok(const KmeansPoints& P, int c) {
  return P.n >= 1 && P.n <= (int64_t)INT_MAX - 64 && P.d4 >= 4 && P.d4 <= kKernMaxDim && !(P.d4 & 3) && P.X &&
         P.nrm && c >= 1 && c <= kKmeansMaxClusters;
}

}  // namespace

KmeansGeometry kmeans_geometry(int64_t n, int d4, int c) {
  KmeansGeometry g;
  constexpr int budget = 8192;   // doubles of partial sums in LDS (64 KiB)
  g.len = (int64_t)c * d4 + c + 2;
  g.cw = std::min(c, std::max(1, budget / d4));
  g.tiles = (c + g.cw - 1) / g.cw;
  g.rl = std::max(1, std::min(256 / d4, budget / (g.cw * d4)));
  int64_t slabs = std::min<int64_t>(512, ceil_div(n, 512));
  slabs = std::max<int64_t>(1, std::min<int64_t>(slabs, ((int64_t)1 << 22) / g.len));
  g.rows_per = ceil_div(n, slabs);
  g.slabs = (int)ceil_div(n, g.rows_per);   // no empty slab
  g.lds_bytes = (g.rl * g.cw * d4 + g.rl) * (int)sizeof(double) + (g.rl * g.cw + g.rl) * (int)sizeof(int);
  return g;
}

bool kmeans_assign(const KmeansPoints& P, int c, const double* C, const double* cnrm, int32_t* label, double* dmin,
                   hipStream_t s) {
  if (!km_shape_ok(P, c) || !C || !cnrm || !dmin) return false;
  switch (kern_ks_cap(P.d4 / 4)) {
    case 1: launch_assign<1>(P.n, P.d4, c, P.X, P.nrm, C, cnrm, label, dmin, s); break;
    case 2: launch_assign<2>(P.n, P.d4, c, P.X, P.nrm, C, cnrm, label, dmin, s); break;
    case 4: launch_assign<4>(P.n, P.d4, c, P.X, P.nrm, C, cnrm, label, dmin, s); break;
    case 8: launch_assign<8>(P.n, P.d4, c, P.X, P.nrm, C, cnrm, label, dmin, s); break;
    case 16: launch_assign<16>(P.n, P.d4, c, P.X, P.nrm, C, cnrm, label, dmin, s); break;
    case 32: launch_assign<32>(P.n, P.d4, c, P.X, P.nrm, C, cnrm, label, dmin, s); break;
    default: launch_assign<64>(P.n, P.d4, c, P.X, P.nrm, C, cnrm, label, dmin, s); break;
  }
  return true;
}

bool kmeans_update(const KmeansPoints& P, int c, const int32_t* label, const int32_t* prev, const double* dmin,
                   double* part, double* tot, hipStream_t s) {
  if (!km_shape_ok(P, c) || !label || !prev || !dmin || !part || !tot) return false;
  const KmeansGeometry g = kmeans_geometry(P.n, P.d4, c);
  // (the attribute is set once per kernel: the largest record any geometry asks for, 8192 doubles of
  // sums, <= 64 inertia partials, <= 2048 counts and <= 64 changed counts)
  ensure_lds_attr(reinterpret_cast<const void*>(&k_kmeans_update), 80 * 1024);
  hipLaunchKernelGGL(k_kmeans_update, dim3((unsigned)g.slabs, (unsigned)g.tiles), dim3(256), g.lds_bytes, s, P.n,
                     P.d4, c, g.cw, g.rl, g.rows_per, P.X, label, prev, dmin, part, g.len);
  reduce_slab(part, g.slabs, g.len, tot, nullptr, s);
  return true;
}

void kmeans_form(int c, int d4, const double* tot, const double* Cold, double* Cnew, double* cnrm_new, double* rec,
                 hipStream_t s) {
  hipLaunchKernelGGL(k_kmeans_form, dim3(1), dim3(256), 0, s, c, d4, tot, Cold, Cnew, rec);
  kernop_norms(c, d4, Cnew, cnrm_new, s);
}

void kmeans_fill_labels(int64_t n, int32_t v, int32_t* label, hipStream_t s) {
  hipLaunchKernelGGL(k_fill_i32, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, n, v, label);
}

int64_t kmeans_seed_slabs(int64_t n) { return ceil_div(n, kSeedSlab); }

bool kmeans_seed_round(const KmeansPoints& P, int r, int64_t last, double u, double* dnew, double* w,
                       double* slabtot, int32_t* picked, hipStream_t s) {
  if (!km_shape_ok(P, 1) || r < 1 || last < 0 || last >= P.n || !dnew || !w || !slabtot || !picked) return false;
  if (!kmeans_assign(P, 1, P.X + last * P.d4, P.nrm + last, nullptr, dnew, s)) return false;
  const int64_t NS = kmeans_seed_slabs(P.n);
  hipLaunchKernelGGL(k_kmeans_seed_round, dim3((unsigned)NS), dim3(256), 0, s, P.n, r == 1 ? 1 : 0, last, dnew, w,
                     slabtot);
  hipLaunchKernelGGL(k_kmeans_seed_pick, dim3(1), dim3(256), 0, s, P.n, NS, w, slabtot, u, r, picked);
  return true;
}

}  // namespace rbl
