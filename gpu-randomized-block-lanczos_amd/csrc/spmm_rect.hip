// spmm_rect.hip — rectangular sparse B (m x n): the device transpose and the gather SpMM pair
// of the implicit normal operator  U = B^T (B Q_i) - Q_{i-1} B_i^T  (images.jl:20-33 runs
// RBL_gpu(transpose(B)*B, k, 1); here B^T B is never formed).
//
// The device holds both orientations as CSR: B (m rows, column ids) and B^T (n rows, row ids).
// Each pass is a gather over one of them — B^T's CSR is the inverted index of B's scatter — so
// no float atomics run and every sum has a fixed order.
//
// Work split (both orientations, any row-length skew): the task table of the segmented gather
// (spmm.hip variant 5) with its own limits: rows of <= kRectSegLen nonzeros are packed into
// wave tasks of <= kRectPack nonzeros and <= 64 rows, longer rows are cut into segments of
// kRectSegLen nonzeros whose partial rows k_rect_fixup sums in segment order.  A lane group of
// BP lanes (the next power of two >= b, at most 64) owns a row; b > 64 runs in 64-column
// chunks.  Output rows differ from input rows, there is no band or tile metadata, and empty
// rows (packed like any short row) are written as zeros (+ the epilogue).
//
// A rank-one shift C = B - u v^T (rbl_set_rect_shift: centring, correspondence analysis,
// deflating a known pair) rides in the epilogue of both passes as out[row, c] -= a[row] w[c]
// with w = X^T (the other shift vector), b values formed on the device by rect_colsum in a
// fixed order, so C^T C is applied with nothing dense formed and no host round trip.
//
// Algorithmic bytes per pass: nnz * 12 + (rows + 1) * 8 + rows * b * 8 (+ n * b * 8 for
// Q_{i-1} in pass 2); the gathered Q rows, nnz * b * 8, are cache traffic.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "kernels.hpp"

namespace rbl {

namespace {

// row of entry e in a CSR row pointer (empty rows skipped): the last r with ptr[r] <= e
__device__ inline int64_t row_of(const int64_t* __restrict__ ptr, int64_t nrows, int64_t e) {
  int64_t lo = 0, hi = nrows;  // ptr[lo] <= e < ptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (ptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- transpose: count per target row, exclusive scan, fill, per-row sort, values ----------
__global__ void k_rect_count(int64_t nnz, const int32_t* __restrict__ ind,
                             unsigned long long* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nnz) atomicAdd(&cnt[ind[e]], 1ull);
}

// slots of a target row handed out through an integer cursor: the row's SET of source ids is
// fixed, only their order is not — the per-row sort that follows fixes it
__global__ void k_rect_fill(int64_t rows, int64_t nnz, const int64_t* __restrict__ ptr,
                            const int32_t* __restrict__ ind, const int64_t* __restrict__ tptr,
                            unsigned long long* __restrict__ cursor, int32_t* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int64_t r = row_of(ptr, rows, e);
  const int32_t t = ind[e];
  const int64_t p = tptr[t] + (int64_t)atomicAdd(&cursor[t], 1ull);
  if (p < tptr[t + 1]) keys[p] = (int32_t)r;
}

// entry p of the transpose, (target row t, source row r = tind[p]): its value is that of
// column t in source row r (rows strictly sorted: binary search)
__global__ void k_rect_values(int64_t cols, int64_t nnz, const int64_t* __restrict__ tptr,
                              const int32_t* __restrict__ tind, const int64_t* __restrict__ ptr,
                              const int32_t* __restrict__ ind, const double* __restrict__ val,
                              double* __restrict__ tval) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nnz) return;
  const int32_t t = (int32_t)row_of(tptr, cols, p);
  const int64_t r = tind[p];
  int64_t lo = ptr[r], hi = ptr[r + 1];  // first entry of row r with ind >= t
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (ind[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  tval[p] = lo < ptr[r + 1] && ind[lo] == t ? val[lo] : 0.0;
}

}  // namespace

int rect_transpose(int64_t rows, int64_t cols, int64_t nnz, const int64_t* ptr, const int32_t* ind,
                   const double* val, int64_t* tptr, int32_t* tind, double* tval, hipStream_t s) {
  unsigned long long* cnt = nullptr;
  int32_t* keys = nullptr;
  void* tmp = nullptr;
  size_t tb_scan = 0, tb_sort = 0;
  const size_t cbytes = (size_t)(cols + 1) * sizeof(unsigned long long);
  hipError_t e = hipMalloc(&cnt, cbytes);
  if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, cbytes, s);
  const unsigned eb = (unsigned)((nnz + 255) / 256);
  if (e == hipSuccess && nnz > 0) {
    hipLaunchKernelGGL(k_rect_count, dim3(eb), dim3(256), 0, s, nnz, ind, cnt);
    e = hipGetLastError();
  }
  const int64_t* cnt_i = reinterpret_cast<const int64_t*>(cnt);
  if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, cnt_i, tptr, cols + 1, s);
  if (e == hipSuccess && nnz > 0) {
    e = hipMalloc(&keys, (size_t)nnz * sizeof(int32_t));
    if (e == hipSuccess)
      e = hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, tb_sort, keys, tind, (int)nnz, (int)cols,
                                                     tptr, tptr + 1, 0, 32, s);
  }
  if (e == hipSuccess) e = hipMalloc(&tmp, std::max<size_t>(std::max(tb_scan, tb_sort), 16));
  if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp, tb_scan, cnt_i, tptr, cols + 1, s);
  if (e == hipSuccess && nnz > 0) {
    e = hipMemsetAsync(cnt, 0, cbytes, s);  // now the fill cursors
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_rect_fill, dim3(eb), dim3(256), 0, s, rows, nnz, ptr, ind, tptr, cnt, keys);
      e = hipGetLastError();
    }
    // every target row's source ids ascending (keys are distinct within a row): the order of
    // SciPy's B.T.tocsr() with sorted indices, whatever order the cursor handed the slots out in
    if (e == hipSuccess)
      e = hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, tb_sort, keys, tind, (int)nnz, (int)cols,
                                                     tptr, tptr + 1, 0, 32, s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_rect_values, dim3(eb), dim3(256), 0, s, cols, nnz, tptr, tind, ptr, ind,
                         val, tval);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(tmp);
  (void)hipFree(keys);
  (void)hipFree(cnt);
  return (int)e;
}

// ----------------------------------------------------------------------------------------
// out[row, c] = (sum_k val[k] Q[ind[k], c]  - sum_u Qprev[row, u] Bi[c, u]) * scale[c]
// for the columns c in [c0, c0 + BP) of b; Q, out, Qprev row-major with leading dimension b.
// SHIFT (sa, sw non-null): the row's sum is followed by  - sa[row] sw[c]  before the Qprev term
// and the scale; empty rows take it like any other, long rows in k_rect_fixup.  Without SHIFT
// the two pointers are unused and the kernel is the unshifted one, instruction for instruction;
// with it the kernel keeps the unshifted one's waves per SIMD (8; 7 at BP = 8).
// ----------------------------------------------------------------------------------------
template <int BP, bool SHIFT>
__global__ __launch_bounds__(256) void k_rect_spmm(
    int64_t ntasks, const int64_t* __restrict__ trow, const int32_t* __restrict__ tinfo,
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ ind,
    const double* __restrict__ val, const double* __restrict__ Q, int b, int c0,
    double* __restrict__ U, double* __restrict__ scratch, const int64_t* __restrict__ slot_k0,
    const double* __restrict__ Qprev, const double* __restrict__ Bi,
    const double* __restrict__ scale, const double* __restrict__ sa,
    const double* __restrict__ sw) {
  constexpr int R = kWave / BP;
  constexpr int G = BP < 8 ? BP : 8;  // Q-row gathers issued back to back per lane group
  // B_i for the epilogue in LDS when it is at most 32 x 32 (bs[u * BP + c] = B_i[c][u]: a lane
  // group reads consecutive words); a 64-lane group (b > 32) reads it from global memory
  constexpr bool kBlds = BP <= 32;
  __shared__ double bs[kBlds ? BP * BP : 1];
  if constexpr (kBlds) {
    if (Qprev)
      for (int e = threadIdx.x; e < b * b; e += 256) bs[(e % b) * BP + e / b] = Bi[e];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ntasks) return;
  const int h = lane / BP, j = lane % BP, c = c0 + j;
  const bool cv = c < b;
  const int cs = cv ? c : c0;
  const int64_t r0 = trow[t];
  const int info = tinfo[t];
  // nonzeros [k, e) of one row, chunks of BP entries (lane j loads entry k + j, coalesced),
  // k stepping by `step`; padding entries gather Q row 0 times 0
  auto dot = [&](int64_t k, int64_t e, int64_t step) -> double {
    double acc0 = 0.0, acc1 = 0.0;
    for (; k < e; k += step) {
      const int64_t kk = k + j;
      const bool ok = kk < e;
      const int cl = ok ? ind[kk] : 0;
      const double vl = ok ? val[kk] : 0.0;
      const int cnt = e - k < BP ? (int)(e - k) : BP;
      for (int j0 = 0; j0 < cnt; j0 += G) {
        double q[G], v[G];
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
          const int cj = __shfl(cl, j0 + jj, BP);
          v[jj] = __shfl(vl, j0 + jj, BP);
          q[jj] = Q[(int64_t)cj * b + cs];
        }
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
          if (jj & 1) acc1 = fma(v[jj], q[jj], acc1);
          else acc0 = fma(v[jj], q[jj], acc0);
        }
      }
    }
    return acc0 + acc1;
  };
  if (info > 0) {
    const double sc = scale ? scale[cs] : 1.0;
    for (int rr = h; rr < info; rr += R) {  // lane-group-uniform row loop
      const int64_t row = r0 + rr;
      double acc = dot(rowptr[row], rowptr[row + 1], BP);
      if constexpr (SHIFT) {
        // sw[c] is read here, after the row's sum, through an index the compiler cannot hoist:
        // held across the row loop it would cost the two registers that decide the occupancy
        int wi = cs;
        asm volatile("" : "+v"(wi));
        acc = fma(-sa[row], sw[wi], acc);
      }
      if (Qprev) {
        if constexpr (kBlds) {
          const double qv = Qprev[row * b + cs];
          for (int u = 0; u < b; ++u) acc = fma(-__shfl(qv, u, BP), bs[u * BP + j], acc);
        } else {
          const double* qp = Qprev + row * b;
          const double* bp = Bi + (int64_t)cs * b;
          for (int u = 0; u < b; ++u) acc = fma(-qp[u], bp[u], acc);
        }
      }
      if (cv) U[row * b + c] = acc * sc;
    }
  } else {
    const int64_t slot = -(int64_t)info - 1;
    const int64_t k0 = slot_k0[slot], k1 = slot_k0[slot + 1];
    const int64_t e = rowptr[r0 + 1] < k1 ? rowptr[r0 + 1] : k1;
    double acc = dot(k0 + (int64_t)h * BP, e, (int64_t)R * BP);
#pragma unroll
    for (int m = BP; m < kWave; m <<= 1) acc += __shfl_xor(acc, m, kWave);
    if (h == 0) scratch[slot * kWave + j] = acc;
  }
}

// long rows: the sum of their segments in slot order, then the epilogue and the scale
template <int BP>
__global__ __launch_bounds__(256) void k_rect_fixup(int64_t nlong, const int64_t* __restrict__ lrow,
                                                   const int64_t* __restrict__ lslot,
                                                   const double* __restrict__ scratch, int b, int c0,
                                                   double* __restrict__ U,
                                                   const double* __restrict__ Qprev,
                                                   const double* __restrict__ Bi,
                                                   const double* __restrict__ scale,
                                                   const double* __restrict__ sa,
                                                   const double* __restrict__ sw) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = g / BP;
  if (i >= nlong) return;
  const int j = (int)(g % BP), c = c0 + j;
  if (c >= b) return;
  const int64_t row = lrow[i];
  double acc = 0.0;
  for (int64_t sl = lslot[i]; sl < lslot[i + 1]; ++sl) acc += scratch[sl * kWave + j];
  if (sa) acc = fma(-sa[row], sw[c], acc);
  if (Qprev)
    for (int u = 0; u < b; ++u) acc = fma(-Qprev[row * b + u], Bi[(int64_t)c * b + u], acc);
  U[row * b + c] = scale ? acc * scale[c] : acc;
}

template <int BP>
static void launch_rect(const CsrDev::Tier& T, const double* Q, int b, int c0, double* out,
                        const double* Qprev, const double* Bi, const double* scale,
                        const double* sa, const double* sw, hipStream_t s) {
  const int64_t blocks = (T.ntasks + 3) / 4;
  if (sa)
    hipLaunchKernelGGL((k_rect_spmm<BP, true>), dim3((unsigned)blocks), dim3(256), 0, s, T.ntasks,
                       T.trow, T.tinfo, T.rowptr, T.col, T.val, Q, b, c0, out, T.scratch, T.slot_k0,
                       Qprev, Bi, scale, sa, sw);
  else
    hipLaunchKernelGGL((k_rect_spmm<BP, false>), dim3((unsigned)blocks), dim3(256), 0, s, T.ntasks,
                       T.trow, T.tinfo, T.rowptr, T.col, T.val, Q, b, c0, out, T.scratch, T.slot_k0,
                       Qprev, Bi, scale, sa, sw);
  if (T.nlong > 0) {
    const int64_t th = T.nlong * BP;
    hipLaunchKernelGGL((k_rect_fixup<BP>), dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s,
                       T.nlong, T.lrow, T.lslot, T.scratch, b, c0, out, Qprev, Bi, scale, sa,
                       sw);
  }
}

void spmm_rect(const CsrDev::Tier& T, const double* Q, int b, double* out, const double* Qprev,
               const double* Bi, const double* scale, hipStream_t s, const double* sa,
               const double* sw) {
  if (T.ntasks <= 0 || b < 1) return;
  if (!sa || !sw) sa = sw = nullptr;
  if (b > 32) {  // 64-lane groups; b > 64 in 64-column chunks (the scratch is reused in stream order)
    for (int c0 = 0; c0 < b; c0 += 64) launch_rect<64>(T, Q, b, c0, out, Qprev, Bi, scale, sa, sw, s);
    return;
  }
  if (b > 16) launch_rect<32>(T, Q, b, 0, out, Qprev, Bi, scale, sa, sw, s);
  else if (b > 8) launch_rect<16>(T, Q, b, 0, out, Qprev, Bi, scale, sa, sw, s);
  else if (b > 4) launch_rect<8>(T, Q, b, 0, out, Qprev, Bi, scale, sa, sw, s);
  else if (b > 2) launch_rect<4>(T, Q, b, 0, out, Qprev, Bi, scale, sa, sw, s);
  else if (b > 1) launch_rect<2>(T, Q, b, 0, out, Qprev, Bi, scale, sa, sw, s);
  else launch_rect<1>(T, Q, b, 0, out, Qprev, Bi, scale, sa, sw, s);
}

// ----------------------------------------------------------------------------------------
// part[g][c] = workgroup g's share of  w[c] = sum_r a[r] X[r, c]  (X row-major rows x b): the
// b-vectors t = Q^T v and s = Y^T u of the shifted operator.  Built as k_cheb_moment
// (spmm_cheb.hip): a row is cw slots of type T (d2v: b / 2 column pairs, 16-byte loads; double:
// b columns), a thread keeps its slot for the whole pass, the workgroup covers a tile of
// nrg = 256 / cw rows at a time (one contiguous stream) and walks the tiles grid-stride; a row
// wider than 256 slots runs in chunks of 256.  Fixed order: each thread over its rows
// ascending, the row groups ascending in LDS, the workgroups by reduce_slab.  No atomics.
// ----------------------------------------------------------------------------------------
namespace {

constexpr int kColsumThreads = 256;
constexpr int kColsumPerCu = 8;  // workgroups per CU (2 waves per SIMD x 4), as the stream passes

int rect_cu_count() {
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

template <typename T>
__global__ __launch_bounds__(kColsumThreads) void k_rect_colsum(int64_t rows, int cw,
                                                                const double* __restrict__ a,
                                                                const T* __restrict__ X,
                                                                double* __restrict__ part) {
  constexpr int VW = sizeof(T) / sizeof(double);  // columns per slot
  __shared__ double sm[VW * kColsumThreads];
  const int cwl = cw < kColsumThreads ? cw : kColsumThreads;  // slots of a row covered at once
  const int nrg = kColsumThreads / cwl;                       // rows per tile
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  double* out = part + (int64_t)blockIdx.x * VW * cw;
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    T acc = T(0.0);
    if (rg < nrg && c < cw)
      for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < rows; r += rstride) acc += a[r] * X[r * cw + c];
    if constexpr (VW == 2) {
      sm[threadIdx.x] = acc.x;
      sm[kColsumThreads + threadIdx.x] = acc.y;
    } else {
      sm[threadIdx.x] = acc;
    }
    __syncthreads();
    const int ncl = cw - cb < cwl ? cw - cb : cwl;  // slots of this chunk
    for (int idx = threadIdx.x; idx < VW * ncl; idx += kColsumThreads) {
      const int v = idx / ncl, c2 = idx % ncl;
      double sum = 0.0;
      for (int g = 0; g < nrg; ++g) sum += sm[v * kColsumThreads + g * cwl + c2];
      out[(cb + c2) * VW + v] = sum;
    }
    __syncthreads();
  }
}

}  // namespace

int rect_colsum_grid(int64_t rows, int b) {
  const int64_t want = (rows * ((b + 1) / 2) + kColsumThreads - 1) / kColsumThreads;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)rect_cu_count() * kColsumPerCu));
}

void rect_colsum(int64_t rows, int b, const double* a, const double* X, double* part, double* w,
                 hipStream_t s) {
  if (rows <= 0 || b < 1) return;
  const int grid = rect_colsum_grid(rows, b);
  // a thread keeps a column pair only when every row starts on a pair: b even, X 16-byte aligned
  if (b % 2 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0)
    hipLaunchKernelGGL((k_rect_colsum<d2v>), dim3(grid), dim3(kColsumThreads), 0, s, rows, b / 2, a,
                       reinterpret_cast<const d2v*>(X), part);
  else
    hipLaunchKernelGGL((k_rect_colsum<double>), dim3(grid), dim3(kColsumThreads), 0, s, rows, b, a, X,
                       part);
  reduce_slab(part, grid, b, w, nullptr, s);
}

}  // namespace rbl
