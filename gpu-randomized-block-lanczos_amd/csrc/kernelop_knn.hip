// kernelop_knn.hip — the k nearest column points of every row point (rbl_kernel_knn):
//
//     row i:  the k smallest of { (d2(i, j), j) : 0 <= j < mc, and j != i in self mode },
//     d2(i, j) = max((|r_i|^2 + |c_j|^2) - 2 r_i.c_j, 0),
//
// in the total order "smaller d2 first, the smaller index on equal d2", written sorted ascending.
// The two point sets and their norms are those of the cross product (kernelop_cross.hip); the inner
// product r_i.c_j is the same fixed-order v_mfma_f64_16x16x4_f64 chain, so in self mode (R and C one
// array) d2(i, j) and d2(j, i) are the same bits.  The kernel function of the operator does not enter.
//
// k_kernop_knn_mfma is the pair-tile scheme of k_kernop_cross_mfma with the second product replaced
// by a selection: a workgroup owns 64 row points (four waves, one 16-row tile each; the R_i fragment
// in registers) and walks stages of JT column points staged through LDS one stage ahead.  In the
// transposed tile P = C_j R_i^T lane (li, q), register r holds row point i0 + li and column point
// j0 + 16 t + q + 4 r: the four lanes q = 0 .. 3 of one li share a row.  Every row's current list (k
// keys, k indices, sorted) lives in LDS and belongs to the wave that owns the row, so the block
// barriers of the stage loop are all the workgroup synchronisation there is; every lane keeps its
// row's k-th entry (the threshold) in registers.  After a tile a lane compares its four candidates
// with the threshold; if no lane of the wave passes — the common case once the lists have filled —
// the wave goes on.  Otherwise the lanes q = 0, 1, 2, 3 take turns (a wave-uniform loop; 16 rows in
// parallel, one lane per row at a time), each inserting its candidates that still pass into the
// row's list, and the wave reloads its thresholds.  LDS operations of one wave complete in order;
// the wavefront-scope fences between the turns keep the compiler from moving the list accesses.
//
// The result is the unique answer of the total order: it depends on neither the insertion order nor
// the split count nor the CU count, there are no atomics, and two calls give the same bits.
//
// The column range is split as the cross product splits it: the grid is ceil(mr / 64) x S, split s
// walks whole stages [st0, st1) and writes its list — padded with (+inf, INT32_MAX) where its range
// holds fewer than k points — to slab s of a scratch; k_kernop_knn_merge, one thread per row, takes
// the k smallest of the S k entries in the same order.  With S = 1 the main kernel writes the result.
#include <algorithm>
#include <climits>
#include <limits>

#include "kernelop_dev.hpp"
#include "kernels.hpp"

namespace rbl {

namespace {

using namespace kerndev;

#ifdef RBL_KNN_COUNT
// diagnostics build only: pair tiles computed by a wave, and those on which any lane inserted
__device__ unsigned long long g_knn_count[2];
#endif

// (d, j) before (td, tj) in the order of the lists
__device__ __forceinline__ bool knn_before(double d, int j, double td, int tj) {
  return d < td || (d == td && j < tj);
}

// what one wave's lanes wrote to its lists is what its other lanes read next
__device__ __forceinline__ void knn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int knn_stage_doubles(int KS) { return 4 * KS * (kern_jt(KS) + 1) + kern_jt(KS); }
// two stage buffers (the X part and the norms), then 64 lists of KC + 1 keys and KC + 1 indices
constexpr int knn_lds_bytes(int KS, int KC) {
  return 2 * knn_stage_doubles(KS) * (int)sizeof(double) + 64 * (KC + 1) * (int)(sizeof(double) + sizeof(int));
}

// KC: the list capacity (k <= KC).  od / oi: the result, mr x k row-major (S = 1), or the slabs of
// the S splits, mr x k each.
template <int KS, int KC>
__global__ __launch_bounds__(256) void k_kernop_knn_mfma(KernKnn op, int ks, double* __restrict__ od,
                                                         int* __restrict__ oi) {
  constexpr int JT = kern_jt(KS);
  constexpr int LDX = JT + 1;            // C_j^T in LDS: element (k, j) at k LDX + j
  constexpr int XPER = JT * 4 * KS / 256;
  constexpr int BUF = knn_stage_doubles(KS);
  constexpr int LDL = KC + 1;            // a list's stride
  extern __shared__ double knn_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int64_t mr = op.mr, mc = op.mc;
  const int d4 = op.d4, k = op.k;
  const int64_t i0 = (int64_t)blockIdx.x * 64 + 16 * wave;
  const int64_t gi = i0 + li;
  const int self = op.self ? (int)gi : -1;   // the column index row gi skips (indices are < 2^31)

  // the wave's R_i fragment and its norm
  double xi[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) xi[kk] = (kk < ks && gi < mr) ? op.R[gi * d4 + 4 * kk + q] : 0.0;
  const double ni = gi < mr ? op.rnrm[gi] : 0.0;

  // this row's list, owned by this wave: rows 16 wave .. 16 wave + 15 of the 64
  double* keys = knn_lds + 2 * BUF + (16 * wave + li) * LDL;
  int* ids = reinterpret_cast<int*>(knn_lds + 2 * BUF + 64 * LDL) + (16 * wave + li) * LDL;
  for (int c = q; c < k; c += 4) {
    keys[c] = std::numeric_limits<double>::infinity();
    ids[c] = INT_MAX;
  }
  double td = std::numeric_limits<double>::infinity();
  int tj = INT_MAX;

  // where this thread's staged elements of C go (the same every stage)
  const int xcount = JT * d4;
  int xofs[XPER];
#pragma unroll
  for (int m = 0; m < XPER; ++m) {
    const int e = tid + 256 * m;
    xofs[m] = e < xcount ? (e % d4) * LDX + e / d4 : -1;
  }
  double xr[XPER], nr = 0.0;
  auto load = [&](int64_t j0) {
#pragma unroll
    for (int m = 0; m < XPER; ++m) {
      const int64_t g = j0 * d4 + tid + 256 * m;
      xr[m] = (xofs[m] >= 0 && g < mc * d4) ? op.C[g] : 0.0;
    }
    if (tid < JT) nr = j0 + tid < mc ? op.cnrm[j0 + tid] : 0.0;
  };
  auto store = [&](double* buf) {
#pragma unroll
    for (int m = 0; m < XPER; ++m)
      if (xofs[m] >= 0) buf[xofs[m]] = xr[m];
    if (tid < JT) buf[4 * KS * LDX + tid] = nr;
  };

  // this split's stages [st0, st1): whole stages, contiguous, the remainder to the first splits
  const int64_t nst = (mc + JT - 1) / JT;
  const int64_t S = gridDim.y, sp = blockIdx.y;
  const int64_t st0 = sp * (nst / S) + (sp < nst % S ? sp : nst % S);
  const int64_t st1 = st0 + nst / S + (sp < nst % S ? 1 : 0);
  if constexpr (KS >= 64) {  // the C rows past d4 of both buffers, which no stage writes: zero
    for (int e = tid; e < 2 * BUF; e += 256)
      if (e % BUF < 4 * KS * LDX) knn_lds[e] = 0.0;
    __syncthreads();
  }
#ifdef RBL_KNN_COUNT
  unsigned ntile = 0, nins = 0;
#endif
  load(st0 * JT);
  store(knn_lds);
  __syncthreads();   // (also: the lists' initial entries, for the lanes that share them)
  for (int64_t s = st0; s < st1; ++s) {
    const int64_t j0 = s * JT;
    if (s + 1 < st1) load(j0 + JT);
    const double* xs = knn_lds + ((s - st0) & 1) * BUF;
    const double* ns = xs + 4 * KS * LDX;
#pragma unroll
    for (int t = 0; t < JT / 16; ++t) {
      if (j0 + 16 * t >= mc) break;  // a pair tile wholly past mc has no candidate
      d4v p = d4v{0.0, 0.0, 0.0, 0.0};
      const double* xt = xs + q * LDX + 16 * t + li;
      if (KS < 64 && ks == KS) {  // (KS = 64: R_i alone fills 128 registers; the guarded form only)
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
      // the four candidates of this lane: column points j0 + 16 t + q + 4 r of row gi
      const int jb = (int)j0 + 16 * t + q;
      double cd[4];
      int pass = 0;   // bit r: candidate r is a real pair and lies before the threshold
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jb + 4 * r;
        cd[r] = fmax((ni + ns[16 * t + q + 4 * r]) - 2.0 * p[r], 0.0);
        if (gi < mr && j < mc && j != self && knn_before(cd[r], j, td, tj)) pass |= 1 << r;
      }
      const bool any = pass != 0;
#ifdef RBL_KNN_COUNT
      ++ntile;
#endif
      if (__ballot(any) == 0ull) continue;
#ifdef RBL_KNN_COUNT
      ++nins;
#endif
      for (int turn = 0; turn < 4; ++turn) {
        if (__ballot(any && q == turn) == 0ull) continue;
        if (any && q == turn) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = jb + 4 * r;
            // the list may have moved since the threshold was loaded: compare with its tail
            if (!(pass >> r & 1) || !knn_before(cd[r], j, keys[k - 1], ids[k - 1])) continue;
            int pos = k - 1;
            while (pos > 0) {
              const double kd = keys[pos - 1];
              const int kj = ids[pos - 1];
              if (!knn_before(cd[r], j, kd, kj)) break;
              keys[pos] = kd;
              ids[pos] = kj;
              --pos;
            }
            keys[pos] = cd[r];
            ids[pos] = j;
          }
        }
        knn_wave_sync();
      }
      td = keys[k - 1];
      tj = ids[k - 1];
    }
    if (s + 1 < st1) store(knn_lds + ((s + 1 - st0) & 1) * BUF);
    __syncthreads();
  }

  // the wave's 16 lists, row-major: to the result, or to this split's slab
  knn_wave_sync();
  const double* wkeys = knn_lds + 2 * BUF + 16 * wave * LDL;
  const int* wids = reinterpret_cast<const int*>(knn_lds + 2 * BUF + 64 * LDL) + 16 * wave * LDL;
  const int64_t base = sp * mr * k;
  for (int e = lane; e < 16 * k; e += 64) {
    const int row = e / k, c = e - row * k;
    if (i0 + row >= mr) break;
    od[base + (i0 + row) * k + c] = wkeys[row * LDL + c];
    oi[base + (i0 + row) * k + c] = wids[row * LDL + c];
  }
#ifdef RBL_KNN_COUNT
  if (lane == 0) {
    atomicAdd(&g_knn_count[0], (unsigned long long)ntile);
    atomicAdd(&g_knn_count[1], (unsigned long long)nins);
  }
#endif
}

// row's k smallest of the S sorted lists pd / pi [s][row][0 .. k), in the order of the lists: a
// merge by the S heads, one thread per row
__global__ __launch_bounds__(256) void k_kernop_knn_merge(const double* __restrict__ pd, const int* __restrict__ pi,
                                                          int S, int64_t mr, int k, double* __restrict__ od,
                                                          int* __restrict__ oi) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= mr) return;
  unsigned char head[kKernCrossMaxSplits];
  for (int s = 0; s < S; ++s) head[s] = 0;
  for (int c = 0; c < k; ++c) {
    double bd = 0.0;
    int bj = 0, bs = -1;
    for (int s = 0; s < S; ++s) {
      if (head[s] >= k) continue;
      const int64_t e = ((int64_t)s * mr + row) * k + head[s];
      const double d = pd[e];
      const int j = pi[e];
      if (bs < 0 || knn_before(d, j, bd, bj)) bd = d, bj = j, bs = s;
    }
    od[row * k + c] = bd;   // bs >= 0: S k >= k entries are left before the c-th pick
    oi[row * k + c] = bj;
    ++head[bs];
  }
}

template <int KS, int KC>
void launch(const KernKnn& op, double* od, int* oi, int S, hipStream_t s) {
  constexpr int lds = knn_lds_bytes(KS, KC);
  ensure_lds_attr(reinterpret_cast<const void*>(&k_kernop_knn_mfma<KS, KC>), lds);
  const dim3 grid((unsigned)ceil_div(op.mr, 64), (unsigned)S);
  hipLaunchKernelGGL((k_kernop_knn_mfma<KS, KC>), grid, dim3(256), lds, s, op, op.d4 / 4, od, oi);
}
template <int KS>
void launch_kc(const KernKnn& op, double* od, int* oi, int S, hipStream_t s) {
  if (op.k <= 16) return launch<KS, 16>(op, od, oi, S, s);
  if (op.k <= 32) return launch<KS, 32>(op, od, oi, S, s);
  return launch<KS, 64>(op, od, oi, S, s);
}

}  // namespace

bool kernop_knn(const KernKnn& op, int32_t* idx, double* d2, int32_t* part_idx, double* part_d2, int splits,
                hipStream_t s) {
  if (op.mr <= 0 || op.mc <= 0 || op.d4 < 4 || op.d4 > kKernMaxDim || (op.d4 & 3) || !op.R || !op.C ||
      !op.rnrm || !op.cnrm || !idx || !d2)
    return false;
  if (op.k < 1 || op.k > kKernKnnMax || op.k > op.mc - (op.self ? 1 : 0)) return false;
  if (op.self && (op.R != op.C || op.mr != op.mc)) return false;
  if (op.mc > (int64_t)INT_MAX - 64 || std::max(op.mr, op.mc) * (int64_t)std::max(op.d4, op.k) >= (int64_t)1 << 40)
    return false;
  const int64_t nst = ceil_div(op.mc, kern_jt(kern_ks_cap(op.d4 / 4)));
  if (splits < 1 || splits > kKernCrossMaxSplits || splits > nst || (splits > 1 && (!part_idx || !part_d2)))
    return false;
  double* od = splits > 1 ? part_d2 : d2;
  int* oi = splits > 1 ? part_idx : idx;
  switch (kern_ks_cap(op.d4 / 4)) {
    case 1: launch_kc<1>(op, od, oi, splits, s); break;
    case 2: launch_kc<2>(op, od, oi, splits, s); break;
    case 4: launch_kc<4>(op, od, oi, splits, s); break;
    case 8: launch_kc<8>(op, od, oi, splits, s); break;
    case 16: launch_kc<16>(op, od, oi, splits, s); break;
    case 32: launch_kc<32>(op, od, oi, splits, s); break;
    default: launch_kc<64>(op, od, oi, splits, s); break;
  }
  if (splits > 1)
    hipLaunchKernelGGL(k_kernop_knn_merge, dim3((unsigned)ceil_div(op.mr, 256)), dim3(256), 0, s, part_d2, part_idx,
                       splits, op.mr, op.k, d2, idx);
  return true;
}

#ifdef RBL_KNN_COUNT
bool kernop_knn_counts(unsigned long long out[2], bool reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_knn_count), 2 * sizeof(unsigned long long)) != hipSuccess) return false;
  const unsigned long long zero[2] = {0ull, 0ull};
  return !reset || hipMemcpyToSymbol(HIP_SYMBOL(g_knn_count), zero, sizeof(zero)) == hipSuccess;
}
#endif

}  // namespace rbl
