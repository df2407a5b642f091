// compress.hip — in-place basis compression of the thick restart (rbl_thick_restart):
//     [X_0 .. X_{p/w-1}]  <-  [X_0 .. X_{m-1}] S        (S: (m w) x p row-major on the device)
// over a run of m row-major n x w panels, the result overwriting the first p / w panels of the
// same run.  No scratch of size n exists: a memory-bounded run has none to give.
//
// In place: a workgroup owns whole rows (every column of every panel of its row tile), keeps the
// accumulators of all p output columns of the tile in registers across the whole k loop, and
// stores only after a workgroup barrier that follows its last load.  No other workgroup reads or
// writes those rows, so no element is overwritten before its last reader has it.
//
// Fast path (w in {16, 32}, v_mfma_f64_16x16x4f64; A[l&15][k=l>>4], B[k=l>>4][l&15], C/D col =
// lane&15, row = (lane>>4) + 4 reg): 64 rows and 4 waves per workgroup, wave v owns the column
// tiles [v CT, v CT + CT) of 16 columns, all four 16-row tiles of them: 16 CT fp64 accumulators per
// lane, 32 CT registers — CT = 8 (p = 512): 256 of the 512 registers a lane has at one wave per
// SIMD, the other half holding the operands, the prefetched panel and the addresses.  That is the
// limit kCompressMaxCols = 512: CT = 12 (p = 768) would leave under 128 registers for the rest.
// Each panel's 64 x w tile (contiguous in memory) is read from HBM once, by 16-byte loads issued
// one panel ahead, and staged through LDS (64 x (w + 2) doubles: the MFMA A reads of a half-wave
// then fall in 32 distinct 8-byte banks); S comes from L2, 16 lanes reading 128 contiguous bytes,
// one k step ahead of its use.  The k loop has no branch: a column tile past p / 16 repeats the
// last valid tile's columns and is not stored.
//
// Generic path (any w, p <= kCompressMaxCols): 8 rows per workgroup, thread t owns the output
// columns t and t + 256 of every row of the tile and loops over the m w inputs.
//
// Every sum runs in ascending k with no atomics: two calls give the same bits.
#include "kernels.hpp"

namespace rbl {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int kCmpRows = 64;     // rows per workgroup, fast path
constexpr int kCmpAnyRows = 8;   // rows per workgroup, generic path

template <int B, int CT>
__global__ __launch_bounds__(256) void k_compress_mfma(int64_t nrows, double* xbase, int64_t stride,
                                                      int m, const double* __restrict__ S, int p) {
  constexpr int LD = B + 2;
  constexpr int NLD = kCmpRows * B / 512;  // 16-byte loads per thread and panel
  __shared__ __attribute__((aligned(16))) double xs[kCmpRows * LD];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kCmpRows;
  const int ntiles = p >> 4;
  // tiles past p / 16 (p no multiple of 64 CT) are computed on the last valid tile's columns and
  // never stored: the k loop stays free of branches
  bool tv[CT];
  int cc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int t = wave * CT + ct;
    tv[ct] = t < ntiles;
    cc[ct] = (tv[ct] ? t : ntiles - 1) * 16 + li;
  }
  d4 acc[4][CT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};

  // element pair e of the tile: row e / (B/2), columns 2 (e % (B/2)) and the next
  d2 pre[NLD];
  auto fetch = [&](int j) {
    const double* src = xbase + (int64_t)j * stride + row0 * B;
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = tid + 256 * u;
      const int r = e / (B / 2);
      pre[u] = row0 + r < nrows ? *reinterpret_cast<const d2*>(src + 2 * e) : d2{0.0, 0.0};
    }
  };
  // S one k step (4 rows of S) ahead of the MFMAs that use it: at one wave per SIMD nothing else
  // hides its L2 latency.  Row kg = 4 t + q of S; past the last step the same rows are re-read.
  const int K = m * B;
  double bcur[CT], bnxt[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) bcur[ct] = S[(int64_t)q * p + cc[ct]];
  fetch(0);
  for (int j = 0; j < m; ++j) {
    __syncthreads();  // the previous panel's MFMA reads of xs are done
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = tid + 256 * u;
      const int r = e / (B / 2), c = 2 * (e % (B / 2));
      *reinterpret_cast<d2*>(xs + r * LD + c) = pre[u];
    }
    __syncthreads();
    if (j + 1 < m) fetch(j + 1);
#pragma unroll
    for (int k0 = 0; k0 < B; k0 += 4) {
      const int kg = j * B + k0 + q;
      const int kn = kg + 4 < K ? kg + 4 : kg;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) bnxt[ct] = S[(int64_t)kn * p + cc[ct]];
      double a[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) a[rt] = xs[(rt * 16 + li) * LD + k0 + q];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
          acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], bcur[ct], acc[rt][ct], 0, 0, 0);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) bcur[ct] = bnxt[ct];
    }
  }
  // In place: every load of this workgroup's rows (all m panels, by all four waves) has been
  // issued and consumed above; no other workgroup touches these rows.  Past this barrier the
  // rows are only written.
  __syncthreads();
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    if (!tv[ct]) continue;
    const int c = cc[ct];
    double* dst = xbase + (int64_t)(c / B) * stride + (c % B);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t r = row0 + rt * 16 + q + 4 * reg;
        if (r < nrows) dst[r * B + 0] = acc[rt][ct][reg];
      }
  }
}

__global__ __launch_bounds__(256) void k_compress_any(int64_t nrows, double* xbase, int64_t stride,
                                                     int m, int w, const double* __restrict__ S,
                                                     int p) {
  constexpr int R = kCmpAnyRows;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(nrows - row0 < R ? nrows - row0 : R);
  const int c0 = tid, c1 = tid + 256;
  const bool v0 = c0 < p, v1 = c1 < p;
  double acc0[R], acc1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc0[r] = acc1[r] = 0.0;
  for (int j = 0; j < m; ++j) {
    const double* xp = xbase + (int64_t)j * stride + row0 * w;
    const double* Sj = S + (int64_t)j * w * p;
    for (int kc = 0; kc < w; ++kc) {
      const double s0 = v0 ? Sj[(int64_t)kc * p + c0] : 0.0;
      const double s1 = v1 ? Sj[(int64_t)kc * p + c1] : 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double x = r < nr ? xp[r * w + kc] : 0.0;
        acc0[r] = fma(x, s0, acc0[r]);
        acc1[r] = fma(x, s1, acc1[r]);
      }
    }
  }
  // In place: every thread of the workgroup has read all m panels of the tile's rows; no other
  // workgroup touches these rows.  Past this barrier the rows are only written.
  __syncthreads();
  if (v0) {
    double* dst = xbase + (int64_t)(c0 / w) * stride + row0 * w + (c0 % w);
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (r < nr) dst[r * w] = acc0[r];
  }
  if (v1) {
    double* dst = xbase + (int64_t)(c1 / w) * stride + row0 * w + (c1 % w);
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (r < nr) dst[r * w] = acc1[r];
  }
}

template <int B>
void launch_mfma(int64_t nrows, double* xb, int64_t stride, int m, const double* S, int p,
                 hipStream_t s) {
  const unsigned wgs = (unsigned)((nrows + kCmpRows - 1) / kCmpRows);
  const int ct = (p / 16 + 3) / 4;
#define RBL_CMP(CT) \
  hipLaunchKernelGGL((k_compress_mfma<B, CT>), dim3(wgs), dim3(256), 0, s, nrows, xb, stride, m, S, p)
  if (ct <= 1) RBL_CMP(1);
  else if (ct <= 2) RBL_CMP(2);
  else if (ct <= 4) RBL_CMP(4);
  else RBL_CMP(8);
#undef RBL_CMP
}

}  // namespace

bool basis_compress_fast(const PanelRun& X, int p) {
  // 16-byte loads of the tile: the run's base and stride keep every panel 16-byte aligned
  return (X.w == 16 || X.w == 32) && p >= X.w && p <= kCompressMaxCols &&
         reinterpret_cast<uintptr_t>(X.base) % 16 == 0 && X.stride % 2 == 0;
}

bool basis_compress(int64_t nrows, const PanelRun& X, const double* S_dev, int p, hipStream_t s,
                    bool generic) {
  if (X.w < 1 || X.count < 1 || p < X.w || p % X.w != 0 || p > kCompressMaxCols ||
      p / X.w > X.count || !X.base)
    return false;
  if (nrows <= 0) return true;
  double* xb = const_cast<double*>(X.base);
  if (!generic && basis_compress_fast(X, p)) {
    if (X.w == 32) launch_mfma<32>(nrows, xb, X.stride, X.count, S_dev, p, s);
    else launch_mfma<16>(nrows, xb, X.stride, X.count, S_dev, p, s);
    return true;
  }
  const unsigned wgs = (unsigned)((nrows + kCmpAnyRows - 1) / kCmpAnyRows);
  hipLaunchKernelGGL(k_compress_any, dim3(wgs), dim3(256), 0, s, nrows, xb, X.stride, X.count, X.w,
                     S_dev, p);
  return true;
}

}  // namespace rbl
