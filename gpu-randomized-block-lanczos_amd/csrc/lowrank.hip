// lowrank.hip — the device passes of an implicit symmetric low-rank update of A (gfx950).
//
// rbl_set_lowrank makes the operator A + P S P^T (P: n x r, S: r x r symmetric, 1 <= r <= 32):
// the modularity matrix A - d d^T / 2m, Hotelling deflation A - V Theta V^T, a double-centred
// kernel matrix H K H.  The dense term is never formed.  After the SpMM (and its fused 3-term
// epilogue) apply_A enqueues, in stream order and with no host round trip,
//
//     w = P^T X          lr_project: k_lr_project + reduce_slab      (rp x b)
//     c = S w            lr_small:   k_lr_small, one workgroup       (rp x b)
//     U[row, :] += P[row, :] c        lr_update: k_lr_update         (rows < n_local only)
//
// P lives on the device row-major with its rows padded with zeros to an even width rp =
// lr_padded_width(r), one of 2, 4, 6, 8, 12, 16, 24, 32, so a row's coefficients are contiguous,
// start on a 16-byte boundary and are loaded two at a time.  X and U are the n x b row-major
// blocks of the Krylov loop.
//
// Both n-sized passes share one thread layout, the one of k_rect_colsum (spmm_rect.hip): a row
// is cw slots of type T (d2v: b / 2 column pairs, 16-byte accesses; double: b columns), a thread
// keeps its slot for the whole pass, the workgroup covers a tile of nrg = 256 / cw rows at a time
// (one contiguous stream of X or U) and walks the tiles grid-stride, the grid sized from the CU
// count and the workgroups of the instantiation that fit a CU; a row wider than 256 slots runs in chunks of 256.  The rp accumulators (project) or the
// slot's rp entries of c (update) sit in registers: the kernels are instantiated for each padded
// width RP, their coefficient loops fully unrolled with no guard.
//
// Every sum has a fixed order — project: each thread over its rows ascending, the workgroup's row
// groups ascending in LDS, the workgroups by reduce_slab; small and update: j ascending — and no
// atomics, so two applications give the same bits.
#include <algorithm>
#include <atomic>

#include "kernels.hpp"

namespace rbl {

namespace {

constexpr int kLrThreads = 256;

int lr_cu_count() {
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

constexpr int kLrPerCu = 8;  // most workgroups per CU (2 waves per SIMD x 4), as the stream passes

// part[g][j][col] = workgroup g's share of w[j][col] = sum_row P[row][j] X[row][col]
template <typename T, int RP>
__global__ __launch_bounds__(kLrThreads) void k_lr_project(int64_t rows, int cw,
                                                           const double* __restrict__ P,
                                                           const T* __restrict__ X,
                                                           double* __restrict__ part) {
  constexpr int VW = sizeof(T) / sizeof(double);  // columns per slot
  constexpr int kRowUnroll = RP <= 8 ? 2 : 1;     // two rows in flight while the registers allow
  __shared__ double sm[VW * kLrThreads];
  const int cwl = cw < kLrThreads ? cw : kLrThreads;  // slots of a row covered at once
  const int nrg = kLrThreads / cwl;                   // rows per tile
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  const int ldw = VW * cw;  // = b
  double* out = part + (int64_t)blockIdx.x * (RP * ldw);
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    T acc[RP];
#pragma unroll
    for (int j = 0; j < RP; ++j) acc[j] = T(0.0);
    if (rg < nrg && c < cw) {
#pragma unroll kRowUnroll
      for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < rows; r += rstride) {
        const T x = X[r * cw + c];
        const d2v* p = reinterpret_cast<const d2v*>(P + r * RP);
#pragma unroll
        for (int j = 0; j < RP; j += 2) {
          const d2v pj = p[j / 2];
          acc[j] += pj.x * x;
          acc[j + 1] += pj.y * x;
        }
      }
    }
    const int ncl = cw - cb < cwl ? cw - cb : cwl;  // slots of this chunk
#pragma unroll
    for (int j = 0; j < RP; ++j) {
      if constexpr (VW == 2) {
        sm[threadIdx.x] = acc[j].x;
        sm[kLrThreads + threadIdx.x] = acc[j].y;
      } else {
        sm[threadIdx.x] = acc[j];
      }
      __syncthreads();
      for (int idx = threadIdx.x; idx < VW * ncl; idx += kLrThreads) {
        const int v = idx / ncl, c2 = idx % ncl;
        double sum = 0.0;
        for (int g = 0; g < nrg; ++g) sum += sm[v * kLrThreads + g * cwl + c2];
        out[j * ldw + (cb + c2) * VW + v] = sum;
      }
      __syncthreads();
    }
  }
}

// c = S w: S r x r row-major, w and c rp x b row-major; the rows r <= i < rp of c are zero
__global__ __launch_bounds__(kLrThreads) void k_lr_small(int r, int rp, int b,
                                                         const double* __restrict__ S,
                                                         const double* __restrict__ w,
                                                         double* __restrict__ c) {
  for (int idx = threadIdx.x; idx < rp * b; idx += kLrThreads) {
    const int i = idx / b, col = idx % b;
    double sum = 0.0;
    if (i < r)
      for (int j = 0; j < r; ++j) sum += S[i * r + j] * w[j * b + col];
    c[idx] = sum;
  }
}

// U[row][col] += sum_j P[row][j] c[j][col], rows < `rows` only
template <typename T, int RP>
__global__ __launch_bounds__(kLrThreads) void k_lr_update(int64_t rows, int cw,
                                                          const double* __restrict__ P,
                                                          const T* __restrict__ C,
                                                          T* __restrict__ U) {
  constexpr int kRowUnroll = RP <= 4 ? 2 : 1;  // wider: a second row in flight costs occupancy
  const int cwl = cw < kLrThreads ? cw : kLrThreads;
  const int nrg = kLrThreads / cwl;
  const int rg = threadIdx.x / cwl, cl = threadIdx.x % cwl;
  const int64_t rstride = (int64_t)gridDim.x * nrg;
  if (rg >= nrg) return;
  for (int cb = 0; cb < cw; cb += cwl) {
    const int c = cb + cl;
    if (c >= cw) continue;
    T cj[RP];
#pragma unroll
    for (int j = 0; j < RP; ++j) cj[j] = C[(int64_t)j * cw + c];
#pragma unroll kRowUnroll
    for (int64_t r = (int64_t)blockIdx.x * nrg + rg; r < rows; r += rstride) {
      const T u = U[r * cw + c];
      const d2v* p = reinterpret_cast<const d2v*>(P + r * RP);
      T t = T(0.0);
#pragma unroll
      for (int j = 0; j < RP; j += 2) {
        const d2v pj = p[j / 2];
        t += pj.x * cj[j];
        t += pj.y * cj[j + 1];
      }
      U[r * cw + c] = u + t;
    }
  }
}

// Workgroups of `kernel` that fit a CU at once, at most kLrPerCu.  The wide instantiations hold
// their accumulators in up to 170 VGPRs and fit fewer; a grid-stride grid larger than what is
// resident leaves its last workgroups to run alone, at a fraction of the bandwidth.  Asked of the
// runtime once per instantiation (every device of a process is the same part).
template <typename K>
int lr_resident(K kernel, std::atomic<int>& cache) {
  int v = cache.load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, kLrThreads, 0) != hipSuccess || v < 1)
      v = 2;
    v = std::min(v, kLrPerCu);
    cache.store(v, std::memory_order_relaxed);
  }
  return v;
}
template <typename T, int RP>
int lr_project_resident() {
  static std::atomic<int> cache{0};
  return lr_resident(k_lr_project<T, RP>, cache);
}
template <typename T, int RP>
int lr_update_resident() {
  static std::atomic<int> cache{0};
  return lr_resident(k_lr_update<T, RP>, cache);
}

int lr_grid_for(int64_t rows, int b, int per_cu) {
  const int64_t want = (rows * ((b + 1) / 2) + kLrThreads - 1) / kLrThreads;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)lr_cu_count() * per_cu));
}

// 16-byte slots only when every row starts on a pair: b even and the block 16-byte aligned
bool lr_pairs(int b, const void* blk) {
  return b % 2 == 0 && (reinterpret_cast<uintptr_t>(blk) & 15) == 0;
}

#define RBL_LR_DISPATCH(LAUNCH) \
  switch (rp) {                 \
    case 2: LAUNCH(2); break;   \
    case 4: LAUNCH(4); break;   \
    case 6: LAUNCH(6); break;   \
    case 8: LAUNCH(8); break;   \
    case 12: LAUNCH(12); break; \
    case 16: LAUNCH(16); break; \
    case 24: LAUNCH(24); break; \
    case 32: LAUNCH(32); break; \
    default: break;             \
  }

}  // namespace

int lr_padded_width(int r) {
  for (int w : {2, 4, 6, 8, 12, 16, 24, 32})
    if (r <= w) return w;
  return 0;
}

// an upper bound of the grid lr_project launches (the partials are sized by it)
int lr_project_grid(int64_t rows, int b, int rp) { return lr_grid_for(rows, b, kLrPerCu); }

void lr_project(int64_t rows, int b, int rp, const double* P, const double* X, double* part,
                double* w, hipStream_t s) {
  if (rows <= 0 || b < 1 || rp != lr_padded_width(rp)) return;
  int grid = 0;
  if (lr_pairs(b, X)) {
#define RBL_LR_PROJ2(RP)                                                                      \
  grid = lr_grid_for(rows, b, lr_project_resident<d2v, RP>());                                \
  hipLaunchKernelGGL((k_lr_project<d2v, RP>), dim3(grid), dim3(kLrThreads), 0, s, rows, b / 2, P, \
                     reinterpret_cast<const d2v*>(X), part)
    RBL_LR_DISPATCH(RBL_LR_PROJ2)
#undef RBL_LR_PROJ2
  } else {
#define RBL_LR_PROJ1(RP)                                                                          \
  grid = lr_grid_for(rows, b, lr_project_resident<double, RP>());                                 \
  hipLaunchKernelGGL((k_lr_project<double, RP>), dim3(grid), dim3(kLrThreads), 0, s, rows, b, P, X, \
                     part)
    RBL_LR_DISPATCH(RBL_LR_PROJ1)
#undef RBL_LR_PROJ1
  }
  reduce_slab(part, grid, (int64_t)rp * b, w, nullptr, s);
}

void lr_small(int r, int rp, int b, const double* S, const double* w, double* c, hipStream_t s) {
  if (r < 1 || b < 1) return;
  hipLaunchKernelGGL(k_lr_small, dim3(1), dim3(kLrThreads), 0, s, r, rp, b, S, w, c);
}

void lr_update(int64_t rows, int b, int rp, const double* P, const double* c, double* U,
               hipStream_t s) {
  if (rows <= 0 || b < 1 || rp != lr_padded_width(rp)) return;
  if (lr_pairs(b, U) && (reinterpret_cast<uintptr_t>(c) & 15) == 0) {
#define RBL_LR_UPD2(RP)                                                                          \
  hipLaunchKernelGGL((k_lr_update<d2v, RP>),                                                     \
                     dim3(lr_grid_for(rows, b, lr_update_resident<d2v, RP>())), dim3(kLrThreads), \
                     0, s, rows, b / 2, P, reinterpret_cast<const d2v*>(c), reinterpret_cast<d2v*>(U))
    RBL_LR_DISPATCH(RBL_LR_UPD2)
#undef RBL_LR_UPD2
  } else {
#define RBL_LR_UPD1(RP)                                                                             \
  hipLaunchKernelGGL((k_lr_update<double, RP>),                                                     \
                     dim3(lr_grid_for(rows, b, lr_update_resident<double, RP>())), dim3(kLrThreads), \
                     0, s, rows, b, P, c, U)
    RBL_LR_DISPATCH(RBL_LR_UPD1)
#undef RBL_LR_UPD1
  }
}

#undef RBL_LR_DISPATCH

}  // namespace rbl
