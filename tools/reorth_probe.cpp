// reorth_probe.cpp — time the shipped partial-reorth kernels (gram44_partial + reduce_slab,
// tsmm44, and at b = 32 the fp32 update tsmm44x32 of RBL_OPT_UPD32 (bf16 MFMA) beside it, plain and in
// its RBL_OPT_UPD32_SHADOW form as a run calls it: the last two panels fresh, the others from the
// fp32 shadow) at n = 1e7, b = 32, X = [Q_i, Q_{i-1}] for a range of basis sizes (diagnostic).
// Build: tools/build_probe.sh (links the library's objects).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../gpu-randomized-block-lanczos_amd/csrc/kernels.hpp"

__global__ void k_fill(double* p, int64_t n, uint64_t seed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    p[i] = ((double)(z >> 11) * 0x1.0p-53 - 0.5) * 1e-2;
  }
}
static void fill(double* p, int64_t n, uint64_t seed) {
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, p, n, seed);
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 10000000;
  // argv: n, b (32 or 16), nWmax (default 36; C3 at b = 16: 1585478 16 72)
  const int b = argc > 2 ? atoi(argv[2]) : 32, nWmax = argc > 3 ? atoi(argv[3]) : 36;
  const int xw = 2 * b;  // X = [Q_i, Q_{i-1}] columns
  double *W, *X0, *X1, *slab, *C, *Cg;
  if (hipMalloc(&W, (size_t)n * b * nWmax * 8) != hipSuccess) return 1;
  (void)hipMalloc(&X0, (size_t)n * b * 8);
  (void)hipMalloc(&X1, (size_t)n * b * 8);
  fill(W, n * b * nWmax, 1);
  fill(X0, n * b, 2);
  fill(X1, n * b, 3);
  size_t slab_elems = 0;  // the split count may depend on nW: size for the largest product
  for (int nW = 2; nW <= nWmax; nW += 2)
    slab_elems = std::max(slab_elems, (size_t)rbl::gram44_splits(n, nW, b) * nW * b * xw);
  (void)hipMalloc(&slab, slab_elems * 8);
  (void)hipMalloc(&C, (size_t)nWmax * b * xw * 8);
  fill(C, nWmax * b * xw, 4);
  (void)hipMalloc(&Cg, (size_t)nWmax * b * xw * 8);
  float* S = nullptr;  // the fp32 shadow of W (b = 32) and its two device counters
  int* cnt = nullptr;
  if (b == 32 && hipMalloc(&S, (size_t)rbl::tsmm44x32_shadow_slot(n) * nWmax * 4) != hipSuccess) return 1;
  if (hipMalloc(&cnt, 2 * sizeof(int)) != hipSuccess) return 1;
  unsigned short* Cp = nullptr;  // the update's split image of C
  if (b == 32 && hipMalloc(&Cp, (size_t)rbl::tsmm44x32_cpieces(nWmax * b) * 2) != hipSuccess) return 1;
  (void)hipMemset(cnt, 0, 2 * sizeof(int));
  // PROBE_XG=1: the update also forms Q_{i-1}^T Q_i (the fused local-reorth Gram)
  const bool xg = getenv("PROBE_XG") && atoi(getenv("PROBE_XG"));
  double* xslab = nullptr;
  int xgrid = 0;
  if (hipMalloc(&xslab, (size_t)rbl::tsmm44_xg_grid(n) * 1024 * 8) != hipSuccess) return 1;
  hipEvent_t e0, e1, e2, e3, e4;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventCreate(&e2);
  (void)hipEventCreate(&e3);
  (void)hipEventCreate(&e4);
  double tg = 0, tt = 0, tu = 0, ts = 0, fl = 0, byg = 0, byt = 0, bys = 0;
  for (int nW = 2; nW <= nWmax; nW += 2) {
    rbl::PanelRun Wr;
    Wr.base = W;
    // PROBE_W0=1: every panel aliases panel 0 (same instruction stream and MFMAs, the basis
    // served from L2 / Infinity Cache instead of HBM) — separates data movement from MFMA issue
    Wr.stride = (getenv("PROBE_W0") && atoi(getenv("PROBE_W0"))) ? 0 : n * b;
    Wr.count = nW;
    Wr.w = b;
    rbl::Panels X;
    X.ptr[0] = X0;
    X.ptr[1] = X1;
    X.count = 2;
    X.w = b;
    const int splits = rbl::gram44_splits(n, nW, b);
    float bg = 1e30f, bt = 1e30f, bu = 1e30f, bs = 1e30f;
    const bool u32 = b == 32 && !xg && rbl::tsmm44x32_ok(n, Wr, X);
    for (int rep = 0; rep < 3; ++rep) {
      (void)hipEventRecord(e0);
      rbl::gram44_partial(n, Wr, X, slab, splits, nullptr, 0);
      rbl::reduce_slab(slab, splits, (int64_t)nW * b * xw, Cg, nullptr, 0);  // C stays fixed: X must not blow up
      (void)hipEventRecord(e1);
      rbl::tsmm44(n, Wr, C, xw, X, -1.0, 1.0, nullptr, 0, xg ? xslab : nullptr, &xgrid);
      (void)hipEventRecord(e2);
      if (u32) rbl::tsmm44x32(n, Wr, C, xw, X, nullptr, Cp, 0);  // the same update in fp32 on bf16 MFMA
      (void)hipEventRecord(e3);
      // the shadow form of a run's even step: panels 0 .. nW - 3 were stored by the earlier sizes
      // of this loop (W never changes here), the last two are fresh
      if (u32 && Wr.stride) rbl::tsmm44x32_shadow(n, Wr, C, xw, X, nullptr, S, nW - 2, cnt, Cp, 0);
      (void)hipEventRecord(e4);
      (void)hipEventSynchronize(e4);
      float g, t, u, sh;
      (void)hipEventElapsedTime(&g, e0, e1);
      (void)hipEventElapsedTime(&t, e1, e2);
      (void)hipEventElapsedTime(&u, e2, e3);
      (void)hipEventElapsedTime(&sh, e3, e4);
      if (rep) {
        bs = sh < bs ? sh : bs;
        bg = g < bg ? g : bg;
        bt = t < bt ? t : bt;
        bu = u < bu ? u : bu;
      }
    }
    const double f = 2.0 * n * nW * b * xw;
    printf("nW=%2d  splits %4d  gram %7.3f ms %5.1f TF   tsmm %7.3f ms %5.1f TF", nW, splits, bg, f / bg / 1e9, bt,
           f / bt / 1e9);
    if (u32) printf("   upd32 %7.3f ms %5.1f TF %5.2f TB/s", bu, f / bu / 1e9, 8.0 * n * (nW * b + 2 * xw) / bu / 1e9);
    if (u32 && Wr.stride) {
      // bytes per row: two fresh fp64 panels, nW - 2 shadow panels read, two written, the pair
      const double gb_basis = 8.0 * n * 2 * b, gb_sh = 4.0 * n * nW * b, gb_pair = 8.0 * n * 2 * xw;
      printf("   shadow %7.3f ms %5.1f TF %5.2f TB/s (basis %.2f shadow %.2f pair %.2f)", bs, f / bs / 1e9,
             (gb_basis + gb_sh + gb_pair) / bs / 1e9, gb_basis / bs / 1e9, gb_sh / bs / 1e9, gb_pair / bs / 1e9);
      ts += bs;
      bys += gb_basis + gb_sh + gb_pair;
    }
    printf("\n");
    if (u32) tu += bu;
    byg += 8.0 * n * (nW * b + xw);       // basis + X read once
    byt += 8.0 * n * (nW * b + 2 * xw);   // basis read, X read and written
    tg += bg;
    tt += bt;
    fl += f;
  }
  printf("sum over nW=2..%d step 2: gram %.1f ms (%.1f TF, %.2f TB/s)  tsmm %.1f ms (%.1f TF, %.2f TB/s)\n", nWmax,
         tg, fl / tg / 1e9, byg / tg / 1e9, tt, fl / tt / 1e9, byt / tt / 1e9);
  if (tu > 0)
    printf("                        upd32 (fp32 sums, bf16 MFMA) %.1f ms (%.1f TF, %.2f TB/s)\n", tu, fl / tu / 1e9, byt / tu / 1e9);
  if (ts > 0)
    printf("                        upd32 with the fp32 shadow %.1f ms (%.1f TF, %.2f TB/s of its own bytes)\n", ts,
           fl / ts / 1e9, bys / ts / 1e9);
  return 0;
}
