// kernelop_cross.hip — the rectangular cross-kernel product (rbl_kernel_cross):
//
//     Y = diag(sr) kappa(R, C) diag(sc) W,    R: mr x d row points, C: mc x d column points,
//
// W mc x b, Y mr x b, both row-major with leading dimension b.  The two point sets are row-major,
// zero-padded to d4 columns, with squared norms from kernop_norms; kappa, gamma, coef0 and degree are
// those of the symmetric operator (kernelop.hip).  There is NO diagonal rule — a row point is never
// "the same point" as a column point, even where the coordinates coincide, so a coincident pair gets
// kappa of the Gram-form distance max(nr + nc - 2 r.c, 0), not exactly kappa(0) — and NO nugget.
//
// k_kernop_cross_mfma is the pair-tile scheme of k_kernop_mfma with rows and columns from two arrays:
// a workgroup owns 64 row points (four waves, one 16-row tile each; the R_i fragment stays in
// registers), walks stages of JT column points staged through LDS one stage ahead, forms the
// TRANSPOSED tile P = C_j R_i^T on v_mfma_f64_16x16x4_f64, applies kappa to its four accumulator
// registers and feeds them as the A operand of the product with W_j (lane maps: kernelop.hip).
//
// Any width runs on MFMA: column chunks of 32 and 16, and a last chunk of 1 .. 15 columns staged
// zero-padded into a 16-column tile, of which only the real columns are written.
//
// The column range is split: the grid is ceil(mr / 64) x S, split s walks a contiguous range of
// whole stages in ascending order (the first nst mod S splits take one stage more) and writes its
// mr x b partial to slab s of a scratch; k_kernop_cross_reduce adds the S partials in ascending s,
// one owner thread per output, and applies sr.  With S = 1 the main kernel writes Y itself.  S comes
// from kernop_cross_splits(mr, mc, d4) alone — never from the device — so the bits do not depend on
// the CU count.  No atomics; two calls give the same bits.
#include <algorithm>

#include "kernelop_dev.hpp"
#include "kernels.hpp"

namespace rbl {

namespace {

using namespace kerndev;

// NB: 16-column tiles of the chunk [c0, c0 + wc), wc <= 16 NB real columns (the rest staged as zeros
// and not written).  part null: Y = sr acc; else slab blockIdx.y of part (mr x ldw each) = acc.
template <int KS, int NB, int KIND>
__global__ __launch_bounds__(256) void k_kernop_cross_mfma(KernCross op, int ks, const double* __restrict__ W,
                                                           int ldw, int c0, int wc, double* __restrict__ Y,
                                                           double* __restrict__ part) {
  constexpr int JT = kern_jt(KS);
  constexpr int LDX = JT + 1;            // C_j^T in LDS: element (k, j) at k LDX + j
  constexpr int WT = 16 * NB;
  constexpr int XPER = JT * 4 * KS / 256;
  constexpr int QPER = JT * WT / 256;
  constexpr int BUF = 4 * KS * LDX + JT * WT + JT;
  extern __shared__ double kern_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int64_t mr = op.mr, mc = op.mc;
  const int d4 = op.d4;
  const int64_t i0 = (int64_t)blockIdx.x * 64 + 16 * wave;
  const int64_t gi = i0 + li;

  // the wave's R_i fragment (B operand of the first product) and its norm
  double xi[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) xi[kk] = (kk < ks && gi < mr) ? op.R[gi * d4 + 4 * kk + q] : 0.0;
  const double ni = gi < mr ? op.rnrm[gi] : 0.0;

  // where this thread's staged elements of C go (the same every stage)
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
      xr[m] = (xofs[m] >= 0 && g < mc * d4) ? op.C[g] : 0.0;
    }
#pragma unroll
    for (int m = 0; m < QPER; ++m) {
      const int e = tid + 256 * m;
      const int64_t j = j0 + e / WT;
      const int c = e % WT;
      double v = 0.0;
      if (j < mc && c < wc) {
        v = W[j * ldw + c0 + c];
        if (op.sc) v *= op.sc[j];
      }
      qr[m] = v;
    }
    if (tid < JT) nr = j0 + tid < mc ? op.cnrm[j0 + tid] : 0.0;
  };
  auto store = [&](double* buf) {
    double* xs = buf;
    double* qs = buf + 4 * KS * LDX;
    double* ns = qs + JT * WT;
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

  // this split's stages [st0, st1): whole stages, contiguous, the remainder to the first splits
  const int64_t nst = (mc + JT - 1) / JT;
  const int64_t S = gridDim.y, sp = blockIdx.y;
  const int64_t st0 = sp * (nst / S) + (sp < nst % S ? sp : nst % S);
  const int64_t st1 = st0 + nst / S + (sp < nst % S ? 1 : 0);
  if constexpr (KS >= 64) {  // the C rows past d4 of both buffers, which no stage writes: zero
    for (int e = tid; e < 2 * BUF; e += 256)
      if (e % BUF < 4 * KS * LDX) kern_lds[e] = 0.0;
    __syncthreads();
  }
  load(st0 * JT);
  store(kern_lds);
  __syncthreads();
  for (int64_t s = st0; s < st1; ++s) {
    const int64_t j0 = s * JT;
    if (s + 1 < st1) load(j0 + JT);
    const double* buf = kern_lds + ((s - st0) & 1) * BUF;
    const double* xs = buf;
    const double* qs = buf + 4 * KS * LDX;
    const double* ns = qs + JT * WT;
#pragma unroll
    for (int t = 0; t < JT / 16; ++t) {
      if (j0 + 16 * t >= mc) break;  // a pair tile wholly past mc adds exact zeros
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
      double kv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        kv[r] = kern_value<KIND>(op.gamma, op.coef0, op.degree, ni, ns[16 * t + q + 4 * r], p[r], false);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ct = 0; ct < NB; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[r], qs[(16 * t + q + 4 * r) * WT + 16 * ct + li],
                                                         acc[ct], 0, 0, 0);
    }
    if (s + 1 < st1) store(kern_lds + ((s + 1 - st0) & 1) * BUF);
    __syncthreads();
  }

  // acc[ct][r]: row i0 + q + 4 r, column c0 + 16 ct + li
  double* out = part ? part + sp * mr * ldw : Y;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = i0 + q + 4 * r;
    if (row >= mr) continue;
    const double si = (!part && op.sr) ? op.sr[row] : 1.0;
#pragma unroll
    for (int ct = 0; ct < NB; ++ct)
      if (16 * ct + li < wc) out[row * ldw + c0 + 16 * ct + li] = si * acc[ct][r];
  }
}

// Y[e] = sr[row] (part[0][e] + part[1][e] + ... + part[S - 1][e]), e = row b + c: ascending s
__global__ __launch_bounds__(256) void k_kernop_cross_reduce(const double* __restrict__ part, int S, int64_t mr,
                                                             int b, const double* __restrict__ sr,
                                                             double* __restrict__ Y) {
  const int64_t len = mr * b;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  double s = part[e];
  for (int k = 1; k < S; ++k) s += part[k * len + e];
  Y[e] = sr ? sr[e / b] * s : s;
}

template <int KS, int NB, int KIND>
void launch_kind(const KernCross& op, const double* W, int ldw, int c0, int wc, double* Y, double* part, int S,
                 hipStream_t s) {
  constexpr int lds = kern_lds_doubles(KS, NB) * (int)sizeof(double);
  ensure_lds_attr(reinterpret_cast<const void*>(&k_kernop_cross_mfma<KS, NB, KIND>), lds);
  const dim3 grid((unsigned)ceil_div(op.mr, 64), (unsigned)S);
  hipLaunchKernelGGL((k_kernop_cross_mfma<KS, NB, KIND>), grid, dim3(256), lds, s, op, op.d4 / 4, W, ldw, c0, wc,
                     Y, part);
}
template <int KS, int NB>
void launch(const KernCross& op, const double* W, int ldw, int c0, int wc, double* Y, double* part, int S,
            hipStream_t s) {
  if (op.kind == kKernRbf) launch_kind<KS, NB, kKernRbf>(op, W, ldw, c0, wc, Y, part, S, s);
  else if (op.kind == kKernLaplace) launch_kind<KS, NB, kKernLaplace>(op, W, ldw, c0, wc, Y, part, S, s);
  else launch_kind<KS, NB, kKernPoly>(op, W, ldw, c0, wc, Y, part, S, s);
}
template <int NB>
void launch_ks(const KernCross& op, const double* W, int ldw, int c0, int wc, double* Y, double* part, int S,
               hipStream_t s) {
  switch (kern_ks_cap(op.d4 / 4)) {
    case 1: return launch<1, NB>(op, W, ldw, c0, wc, Y, part, S, s);
    case 2: return launch<2, NB>(op, W, ldw, c0, wc, Y, part, S, s);
    case 4: return launch<4, NB>(op, W, ldw, c0, wc, Y, part, S, s);
    case 8: return launch<8, NB>(op, W, ldw, c0, wc, Y, part, S, s);
    case 16: return launch<16, NB>(op, W, ldw, c0, wc, Y, part, S, s);
    case 32: return launch<32, NB>(op, W, ldw, c0, wc, Y, part, S, s);
    default: return launch<64, NB>(op, W, ldw, c0, wc, Y, part, S, s);
  }
}

}  // namespace

int kernop_cross_splits(int64_t mr, int64_t mc, int d4) {
  if (mr < 1 || mc < 1 || d4 < 4) return 1;
  const int64_t blocks = ceil_div(mr, 64);
  const int64_t nst = ceil_div(mc, kern_jt(kern_ks_cap(d4 / 4)));
  const int64_t want = ceil_div(kKernCrossWorkgroups, blocks);  // 1 once the rows alone fill the target
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)kKernCrossMaxSplits, nst / kKernCrossMinStages}));
}

bool kernop_cross(const KernCross& op, const double* W, int b, double* Y, double* part, int splits,
                  hipStream_t s) {
  if (op.mr <= 0 || op.mc <= 0 || b < 1 || op.d4 < 4 || op.d4 > kKernMaxDim || (op.d4 & 3) || !op.R || !op.C ||
      !op.rnrm || !op.cnrm)
    return false;
  if (std::max(op.mr, op.mc) * (int64_t)std::max(op.d4, b) >= (int64_t)1 << 40) return false;
  const int64_t nst = ceil_div(op.mc, kern_jt(kern_ks_cap(op.d4 / 4)));
  if (splits < 1 || splits > kKernCrossMaxSplits || splits > nst || (splits > 1 && !part)) return false;
  double* slab = splits > 1 ? part : nullptr;
  int c0 = 0;
  for (; b - c0 >= 32; c0 += 32) launch_ks<2>(op, W, b, c0, 32, Y, slab, splits, s);
  for (; c0 < b; c0 += 16) launch_ks<1>(op, W, b, c0, std::min(16, b - c0), Y, slab, splits, s);
  if (splits > 1)
    hipLaunchKernelGGL(k_kernop_cross_reduce, dim3((unsigned)ceil_div(op.mr * b, 256)), dim3(256), 0, s, slab,
                       splits, op.mr, b, op.sr, Y);
  return true;
}

}  // namespace rbl
