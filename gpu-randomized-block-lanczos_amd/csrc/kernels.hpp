// kernels.hpp — host launchers for the gfx950 RBL kernels (implemented in *.hip).
#pragma once
#include "rbl_common.hpp"

namespace rbl {

// A list of n x w row-major panels ("blocks"): panel t starts at ptr[t] (t < count).
// Used for Krylov blocks (w = b), the pair [Q_i, Q_{i-1}] and the Ritz output (w = k).
struct Panels {
  static constexpr int kMax = 2;
  const double* ptr[kMax] = {nullptr, nullptr};
  int count = 0;
  int w = 0;              // width of each panel (leading dimension = w)
};
// Contiguous run of `count` panels of width w, panel j at base + j*stride (Krylov basis).
struct PanelRun {
  const double* base = nullptr;
  const float* base32 = nullptr;  // fp32 panels instead (tsmm44_f32x only)
  int64_t stride = 0;
  int count = 0;
  int w = 0;
};

// CSR rows [0,nrows) of the local slice; columns are global ids; Q row c lives at
// Qin + (c - col_off) * b.
// Device CSR arrays carry kCsrPad zero entries past nnz, and every n x b buffer an SpMM
// writes carries kRowPad spare rows: the band kernel's loads and stores run unguarded.
constexpr int64_t kCsrPad = 256;
constexpr int64_t kRowPad = 16;
// zeroed rows past the fp32 basis slots and the fp32 staging slot: the fp32 Gram's shifted
// chunks (reorth32.hip, up to this many rows) may read them when a slice has fewer rows
constexpr int64_t kRowPad32 = 32;

struct CsrDev {
  int64_t nrows = 0;
  int64_t nnz = 0;
  const int64_t* rowptr = nullptr;
  const int32_t* col = nullptr;
  const double* val = nullptr;
  // LDS-window metadata (16-row tiles): forward-filled min/max column per tile, and
  // whether every tile fits the window kernel's ring for b = 16 / b = 32.
  const int64_t* tile_cmin = nullptr;
  const int64_t* tile_cmax = nullptr;
  // per tile: e0, nnz, lo, hi (ring rows the tile adds), cmin, cmax, 0, 0
  const int64_t* tile_info = nullptr;
  int64_t ntiles = 0;
  int64_t tiles_per_wg = 0;
  // column-panel SpMM (spmm_panel.hip, b = 32): per block of panel_rows() local rows its first
  // and last panel of panel_width() Q rows (global ids); null: not applicable
  const int32_t* panel_blk = nullptr;   // per block: first / last panel, count offset (int64)
  const uint16_t* panel_cnt = nullptr;  // per block, panel and row: the row's entries there
  const uint32_t* panel_st = nullptr;   // ... and where they start (records from the block's base)
  const uint8_t* panel_col = nullptr;   // the records, panel-major within a block: column - panel
  const double* panel_val = nullptr;    //   base (one byte), value
  int64_t panel_nblk = 0;
  int panel_rpg = 4;         // rows per 16-lane group (blocks of 64 rpg rows): 4 or 8
  int panel_ch = 32;         // records per row and chunk load: 16 or 32
  bool panel_auto = false;   // the automatic choice takes it (else only when forced)
  bool window_ok16 = false;
  bool window_ok32 = false;
  bool band_ok16 = false;   // spmm_band.hip applicable (and dense enough to pay)
  bool band_ok32 = false;
  bool band_gram = false;   // every tile's own rows lie in its band window (ring-resident)
  bool band_pair = false;   // every tile-row pair (2p, 2p+1) has <= 253 nonzeros
  int64_t row0 = 0;         // global index of local row 0 (row-partitioned runs)
  // band kernel: per nonzero, its byte offset in the tile's dense LDS band
  // ((row % 16) * kBandLd + perm8(col - c16(tile))) * 8 (band_positions; kCsrPad entries past nnz)
  const uint16_t* band_pos = nullptr;
  // band-tile kernel (spmm_bt.hip): the CSR densified into MFMA-ordered 16-row tiles with
  // band groups NG = (2H+16)/16 (0: not applicable), and the Q rows the kernel may read
  // (global [q_lo, q_hi); other band rows read zrow, 32 zeros)
  const double* bt = nullptr;
  int bt_ng = 0;
  int64_t bt_tiles_per_wg = 0;
  int64_t q_lo = 0, q_hi = 0;
  const double* zrow = nullptr;
  // several ranks: the own rows [loc_lo, loc_hi) read straight from the block (fp64, or fp32
  // on the fp32-basis path) instead of from Qin, whose halo buffer then holds only the
  // neighbours' rows — no per-step copy of the local block.  Band-tile kernel only: spmm()
  // fails if another kernel would run with qloc set.
  const void* qloc = nullptr;
  int64_t loc_lo = 0, loc_hi = 0;
  // local reorth fused into the band-tile SpMM (RBL_OPT_FUSE bit 2, b = 32, dense tiles; one
  // rank or several — then each rank's edge rows are corrected before the halo exchange, by
  // spmm_bt_locfix_edges, and the SpMM leaves them as read): the kernel stages every Q ring row as Q_i - Q_{i-1} C (C = lfix_c, b x b on the
  // device; Q_{i-1} = the SpMM's Qprev) and writes the corrected own rows back into lfix_q
  // (the block Q_i) except the first and last H rows of each workgroup's range, which
  // neighbours read raw — spmm_bt_locfix_rest corrects those after the SpMM
  // (spmm_bt_locfix_ok: applicable; spmm_bt_locfix_edges: the rank-edge rows beforehand)
  const double* lfix_c = nullptr;
  double* lfix_q = nullptr;
  int* two_wave = nullptr;          // set to 1 when the two-waves-per-SIMD kernel (k_spmm_bt2) ran
  int64_t lfix_lo = 0, lfix_hi = 0;  // local rows still raw (several ranks: the rank's first and
                                     // last H rows were corrected before the halo exchange)
  // packed band tiles (bt_pack): per tile slot a header of bt_pack_words(NG) 8-B words (per
  // 1-KiB operand block the nonzero masks of element 0 / 1 of every lane, then the blocks'
  // uint16 start offsets + the tile's count, then the tile's first value index) and the
  // nonzeros per block: element 0 of the lanes, then element 1; null: the dense tiles `bt`
  const uint64_t* btp_hdr = nullptr;
  const double* btp_val = nullptr;
  // half band tiles (A symmetric, bt_half): groups NGL..NG-1 of every tile slot, and the
  // first NGL local tiles whole; replaces `bt`
  const double* bth = nullptr;
  const double* bte = nullptr;
  // segmented gather (spmm.hip variant 5): wave tasks (first row, info: > 0 rows of a packed
  // short-row task, < 0 -(slot+1) of a long-row segment), segment slots' first nonzero
  // (slot_k0, nslots + 1 entries), long rows with their first slot (lslot, nlong + 1), and a
  // scratch of nslots x 32 partial rows
  int64_t seg_ntasks = 0;
  const int64_t* seg_trow = nullptr;
  const int32_t* seg_tinfo = nullptr;
  const int64_t* seg_slot_k0 = nullptr;
  int64_t seg_nlong = 0;
  const int64_t* seg_lrow = nullptr;
  const int64_t* seg_lslot = nullptr;
  double* seg_scratch = nullptr;
  // column tiers of the segmented gather (RBL_SEG_TIERS; one rank): the nonzeros split by the
  // degree rank of their column into up to kMaxSegTiers CSRs of the same rows, each with its
  // own task table; the SpMM sweeps them in order, accumulating into U, so each sweep's Q-row
  // gathers come from a set that fits a cache level (hot rows: an XCD's L2)
  int seg_ntiers = 0;
  // several ranks: two tiers, the own columns [loc_lo, loc_hi) (tier 0, gathered from `qloc`,
  // the block itself, when set) and the halo columns (tier 1, from Qin): tier 0 runs while the
  // halo exchange is in flight; the stream waits for `seg_wait` (if set) before tier 1
  bool seg_split = false;
  hipEvent_t seg_wait = nullptr;
  struct Tier {
    const int64_t* rowptr = nullptr;
    const int32_t* col = nullptr;
    const double* val = nullptr;
    int64_t ntasks = 0, nlong = 0;
    const int64_t* trow = nullptr;
    const int32_t* tinfo = nullptr;
    const int64_t* slot_k0 = nullptr;
    const int64_t* lrow = nullptr;
    const int64_t* lslot = nullptr;
    double* scratch = nullptr;
  } seg_tier[3];
};
constexpr int kMaxSegTiers = 3;
constexpr int64_t kSegLen = 4096;   // nonzeros per long-row segment
constexpr int64_t kSegPack = 512;   // nonzeros per packed short-row task (<= 64 rows)

// --- rowop.hip ---------------------------------------------------------------------------
// Y' = beta Y + alpha X C (X, Y: n x b panels, C: b x b row-major, ldc) in one pass, and if
// slab != null the Gram Y'^T Y' as grid partials slab[grid][b][b] (reduce with reduce_slab).
// X may equal Y (in place).  b in {16, 32}.
bool rowgram_ok(int b);
int rowgram_grid(int64_t nrows, int per_cu = 2);
constexpr int kRowgramMaxPerCu = 4;  // rowgram_ex's grids stay <= rowgram_grid(nrows, this)
// X32 (optional): X read from fp32 instead (widened exactly).  Y32 (optional): Y' written to
// Y32 rounded to fp32 instead of Y — unless f64flag is non-null and *f64flag != 0 (device).
// tri: C is upper triangular (zeros below the diagonal), X fp64 — all-zero MFMA blocks skipped.
void rowgram(int64_t nrows, int b, const double* X, const double* C, int ldc, double* Y,
             double alpha, double beta, double* slab, int grid, const int* skip, hipStream_t s,
             const float* X32 = nullptr, float* Y32 = nullptr, const int* f64flag = nullptr,
             bool tri = false);
// The CholQR forms of the fused row op (b in {16, 32}, X fp64):
//   mode 1: slab <- Gram of X C (no store);  mode 2: Y = (X C) C2 (slab must be null);
//   Z != null (modes 0 and 2): slab2 <- per-workgroup partials of Z^T Y (grid x b x b).
// grid <= 0: as many persistent workgroups as the instantiation keeps resident (its register
// budget), reported in *grid_out.  Returns false for an unsupported combination.
struct RowOpArgs {
  const double* X = nullptr;
  const double* C = nullptr;
  int ldc = 0;
  double* Y = nullptr;
  double alpha = 1.0, beta = 0.0;
  double* slab = nullptr;
  const int* skip = nullptr;
  const float* X32 = nullptr;
  float* Y32 = nullptr;
  const int* f64flag = nullptr;
  const double* C2 = nullptr;
  const double* Z = nullptr;
  double* slab2 = nullptr;
  int mode = 0;
  int* grid_out = nullptr;  // rowgram_ex with grid <= 0: the grid it chose (per-CU occupancy)
  bool tri = false;         // C (and C2) upper triangular: all-zero MFMA blocks skipped (exact)
};
bool rowgram_ex(int64_t nrows, int b, const RowOpArgs& a, int grid, hipStream_t s);

// --- spmm.hip ----------------------------------------------------------------------------
// U = A * Qin  (+ epilogue U -= Qprev * Bt^T with Bt = B_i row-major b x b, if Qprev).
// variant: 0 auto, 1 global gather, 2 LDS window, 3 LDS band (MFMA), 4 band tiles (MFMA),
// 5 segmented gather (b in {16, 32}).
// ai_slab: if non-null and the band kernel runs with band_gram, it also forms the partials
// of A_i = Qin[own rows]^T U (b x b per workgroup) there; returns how many (0: not formed).
int spmm(const CsrDev& A, const double* Qin, int64_t col_off, int b, double* U,
         const double* Qprev, const double* Bi, int variant, hipStream_t s,
         double* ai_slab = nullptr);

bool spmm_seg_ok(const CsrDev& A, int b);
// column tiers (CsrDev::seg_tier): per row, the nonzeros of each tier (tier_of[col], uint8)
// counted into cnt[t * m + r], then copied in column order into the tier CSRs
void seg_tier_count(int64_t m, const int64_t* rowptr, const int32_t* col, const uint8_t* tier_of,
                    int ntiers, int32_t* cnt, hipStream_t s);
void seg_tier_fill(int64_t m, const int64_t* rowptr, const int32_t* col, const double* val,
                   const uint8_t* tier_of, int ntiers, int64_t* const* trp, int32_t* const* tcol,
                   double* const* tval, hipStream_t s);
// The same by a per-nonzero rule instead of tier_of[col] (TierRule: several ranks, the halo split
// into pulled and pushed products — rbl_api.cpp prepare_tiers): local row r (global row0 + r),
// column c: tier 0 if c is an own row; else tier 1 if c ranks above r — (deg[c], c) >
// (deg[r], r), deg indexed by global id — (the rank pulls Q_c); else tier 2 (the owner of c
// computes the product and pushes it).
struct TierRule {
  const int32_t* deg = nullptr;  // n entries (device); null: use tier_of
  int64_t row0 = 0, r0 = 0, r1 = 0;
};
void seg_tier_count_rule(int64_t m, const int64_t* rowptr, const int32_t* col, TierRule rule,
                         int32_t* cnt, hipStream_t s);
void seg_tier_fill_rule(int64_t m, const int64_t* rowptr, const int32_t* col, const double* val,
                        TierRule rule, int64_t* const* trp, int32_t* const* tcol,
                        double* const* tval, hipStream_t s);
// One tier as a plain CSR product: out[row] = sum_k val[k] Q[col[k] - col_off] (no epilogue),
// b in {16, 32} — the pushed partial rows of the halo split.
void spmm_seg_tier(const CsrDev::Tier& T, const double* Q, int64_t col_off, int b, double* out,
                   hipStream_t s);
// U[rows[i]] += sum_{k in [ptr[i], ptr[i+1])} recv[slot[k]] (slots in order: deterministic), b
// columns — the received pushed partials added to their rows.
void push_add(const int64_t* rows, const int64_t* ptr, const int64_t* slot, int64_t nrows,
              const double* recv, int b, double* U, hipStream_t s);
// --- spmm_rect.hip: rectangular sparse B (rbl_set_matrix_normal) ---------------------------
// One orientation of B is a CSR with its task table (a CsrDev::Tier: rows packed / cut as for
// the segmented gather, with these limits; scratch holds kWave doubles per segment slot).
constexpr int64_t kRectSegLen = 1024;  // nonzeros per long-row segment
constexpr int64_t kRectPack = 512;     // nonzeros per packed short-row task (<= 64 rows)
// The other orientation of a CSR (`rows` rows, ids < cols, every row strictly ascending), built
// on the device: tptr (cols + 1), tind / tval (nnz), every row of the result ascending — the
// same arrays whatever order the fill ran in.  nnz < 2^31.  Returns 0 or a hipError_t.
int rect_transpose(int64_t rows, int64_t cols, int64_t nnz, const int64_t* ptr, const int32_t* ind,
                   const double* val, int64_t* tptr, int32_t* tind, double* tval, hipStream_t s);
// out = T Q (- sa sw^T if sa) (- Qprev Bi^T if Qprev) (columns scaled by scale[c] if scale): Q,
// out, Qprev row-major with b columns, any b >= 1; out has T's rows, Q the rows T's ids index.
// sa / sw: the rank-one shift of rbl_set_rect_shift, out[row][c] -= sa[row] * sw[c] (sa: one
// entry per row of T, sw: b entries, both on the device; both null: no shift, the arithmetic of
// the unshifted pass).  Empty rows receive it, long rows once in the fix-up.
void spmm_rect(const CsrDev::Tier& T, const double* Q, int b, double* out, const double* Qprev,
               const double* Bi, const double* scale, hipStream_t s, const double* sa = nullptr,
               const double* sw = nullptr);
// w[c] = sum_r a[r] X[r][c], c < b: the weighted column sums of a row-major rows x b block
// (t = Q^T v and s = Y^T u of the shifted operator), 1 <= b <= RBL_MAX_BLOCK.  part holds
// rect_colsum_grid(rows, b) x b doubles (per-workgroup partials, added by reduce_slab); a fixed
// summation order, no atomics; 16-byte loads when b is even and X is 16-byte aligned.
int rect_colsum_grid(int64_t rows, int b);
void rect_colsum(int64_t rows, int b, const double* a, const double* X, double* part, double* w,
                 hipStream_t s);
// spmm_panel.hip: column-panel CSR kernel for wide bands (b = 32, Q rows [q_lo, q_hi)); false
// if not applicable.  panel_width(): Q rows per panel.
bool spmm_panel(const CsrDev& A, const double* Qin, int64_t col_off, int b, double* U,
                const double* Qprev, const double* Bi, hipStream_t s);
int panel_width();
// the column-panel format (zeroed and filled on the device, stream-ordered): every row's count
// (cnt) and first record (st) in every panel of its block's window, and the records themselves
// regrouped panel-major within each block (pcol: column within the panel, pval: value); binfo
// on the device; ncnt entries of cnt / st, nnz records
int panel_format(const CsrDev& A, const int32_t* binfo, int R, int64_t nblk, uint16_t* cnt,
                 uint32_t* st, int64_t ncnt, uint8_t* pcol, double* pval, hipStream_t s);
// spmm_window.hip: persistent LDS-window kernel (b in {16,32}); false if not applicable.
bool spmm_window(const CsrDev& A, const double* Qin, int64_t col_off, int b, double* U,
                 const double* Qprev, const double* Bi, hipStream_t s);
int window_grid();              // workgroups for the window kernel (= CUs)
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel): thread-safe
// (in-process ranks launch from several threads) and per device (a process may drive several)
void ensure_lds_attr(const void* kernel, int bytes);
// spmm_band.hip: LDS-densified band tiles on fp64 MFMA (b in {16,32}); false if not applicable.
// ai_slab / ai_parts: see spmm().
bool spmm_band(const CsrDev& A, const double* Qin, int64_t col_off, int b, double* U,
               const double* Qprev, const double* Bi, hipStream_t s, double* ai_slab = nullptr,
               int* ai_parts = nullptr);
// spmm_bt.hip: band tiles in MFMA operand order streamed to VGPRs (b = 32, H in {32, 64});
// false if not applicable.
// Q32 / Qprev32 (optional, the fp32 basis): read fp32 blocks instead of Qin / Qprev.
bool spmm_bt_locfix_ok(const CsrDev& A, int b);
int spmm_bt_halfwidth(const CsrDev& A);
void spmm_bt_locfix_edges(const CsrDev& A, double* Q, const double* Qprev, const double* C,
                          int64_t lo0, int64_t hi0, int64_t lo1, int64_t hi1, hipStream_t s);
void spmm_bt_locfix_rest(const CsrDev& A, double* Q, const double* Qprev, const double* C,
                         hipStream_t s);
bool spmm_bt(const CsrDev& A, const double* Qin, int64_t col_off, int b, double* U,
             const double* Qprev, const double* Bi, hipStream_t s, double* ai_slab = nullptr,
             int* ai_parts = nullptr, const float* Q32 = nullptr, const float* Qprev32 = nullptr);
// band-tile format of the local CSR: tiles in consumption order (slot (round * grid + wg) * 4
// + wave), zero-filled `out` of bt_tile_slots(ntiles, tiles_per_wg) * NG * 256 doubles
// half tiles from the whole ones when the tiles are symmetric bit for bit (0; -1: not
// symmetric, nothing allocated; > 0: HIP error)
int bt_half(const double* full, int64_t ntiles, int64_t tpw, int NG, double** half,
            double** edge, hipStream_t s);
int64_t bt_tile_slots(int64_t ntiles, int64_t tiles_per_wg);
void bt_fill(const CsrDev& A, int H, int NG, double* out, hipStream_t s);
// packed band tiles from the dense ones (NG in {5, 9}): header words per tile slot, and the
// packed values (allocated here, *val_out; *nval_out values); returns 0 or a hipError_t
constexpr int bt_pack_words(int NG) { return (4 * NG + (2 * NG + 4) / 4 + 2) & ~1; }
int bt_pack(const double* dense, int64_t nslots, int NG, uint64_t* hdr, double** val_out,
            int64_t* nval_out, hipStream_t s);
constexpr int kWindowTileRows = 16;
// Band kernel geometry (host checks in rbl_api.cpp): a tile's band [c16, cmax] with
// c16 = cmin & ~15 spans <= kBandMaxK columns; the Q ring holds kBandRing rows; per tile a
// producer pass stores ring rows in whole sets of 512 / b (one element per producer thread).
constexpr int kBandMaxK = 176;
constexpr int kBandLd = 196;
constexpr int kBandRing = 256;
// positions of every nonzero in its tile's dense band (CsrDev::band_pos), from tile_info
void band_positions(const CsrDev& A, uint16_t* pos, hipStream_t s);

// --- spmm_cheb.hip: row passes of the Chebyshev-filtered operator and of Rayleigh-Ritz on A --
// out = alpha W + beta Y (+ gamma Z if Z) over `len` contiguous doubles (an n x b row-major
// block): one term of the filter recurrence after its SpMM.  out may be W.  Any len >= 0; 16-byte
// accesses when every pointer is 16-byte aligned; the grid follows the CU count.
void cheb_axpby(int64_t len, const double* W, const double* Y, const double* Z, double alpha,
                double beta, double gamma, double* out, hipStream_t s);
// One term of a Chebyshev series after its SpMM W = A T_{j-1}, fused with the accumulation:
//   T_j = alpha W + beta T1 (- T2 unless first);  ACC += mu T_j  (first: ACC = mu0 T1 + mu T_j,
//   ACC not read);  T_j stored to Tout unless last (Tout may be W; ACC aliases nothing).
// Same stream conventions as cheb_axpby (16-byte form when every pointer used is 16-byte
// aligned, guarded odd tail, grid from the CU count, no atomics).
void cheb_series_term(int64_t len, const double* W, const double* T1, const double* T2, double alpha,
                      double beta, double mu, double mu0, double* Tout, double* ACC, bool first,
                      bool last, hipStream_t s);
// One term of the Chebyshev moments after its SpMM W = A t_{j-1} (n x b row-major blocks):
//   t_j = alpha W + beta T1 (- T2 unless first), stored to Tout unless last (Tout may be W), and
//   part[g][q][c], g < grid = moment_grid(nrows, b), c < b: workgroup g's partial column sums
//   q = 0: <t_j,t_j>, q = 1: <t_j,T1>, and if first q = 2: <T1,T1>  (2b or 3b doubles per g).
// A fixed summation order, no atomics; reduce_slab over the grid gives the dots.  16-byte
// accesses when b is even and every pointer used is 16-byte aligned, else 8-byte.
int moment_grid(int64_t nrows, int b);
void cheb_moment_term(int64_t nrows, int b, const double* W, const double* T1, const double* T2,
                      double alpha, double beta, double* Tout, double* part, int grid, bool first,
                      bool last, hipStream_t s);
// One term of the diagonal recurrence (rbl_cheb_diag) after its SpMM W = A t_{j-1} (n x b
// row-major blocks, 1 <= b <= 256: a row is finished inside one tile pass of the workgroup, so no
// cross-chunk row accumulation exists; a wider b is not launched):
//   t_j = alpha W + beta T1 (- T2 unless first), stored to Tout unless last (Tout may be W);
//   s[row] = sum_c X[row][c] t_j[row][c];   D[row][e] += coef[e] s[row], e < nf (D: n x nf row-major,
//   coef: this term's nf coefficients, on the device);
//   first (T1 = X; T1, T2 not read; coef: the 2 nf coefficients of terms 0 and 1): q[row] = sum_c
//   X[row][c]^2, qout[row] = q, D[row][e] = coef[e] q + coef[nf + e] s (D not read).
// The row sums run in a fixed order (each thread its slot's columns, the row's slots ascending
// through LDS, one owner thread per element of D): no atomics, two calls give the same bits.
// 16-byte accesses when b is even and every pointer used is 16-byte aligned, else 8-byte.
void cheb_diag_term(int64_t nrows, int b, int nf, const double* W, const double* T1, const double* T2,
                    const double* X, double alpha, double beta, double* Tout, const double* coef,
                    double* D, double* qout, bool first, bool last, hipStream_t s);
// x[i] = x[i] < 0 ? -1 : +1 in place over `len` doubles (0 -> +1): the signs of an N(0,1) block
void sign_block(int64_t len, double* x, hipStream_t s);
// part[g][c] = sum over workgroup g's rows of (Z[r][c] - X[r][c] theta[c])^2, c < kp (Z, X: n x kp
// row-major), g < grid = resid_grid(nrows): a fixed summation order, no atomics; reduce_slab
// over the grid gives the squared column norms.
int resid_grid(int64_t nrows);
void resid_partial(int64_t nrows, int kp, const double* Z, const double* X, const double* theta,
                   double* part, int grid, hipStream_t s);
// dst[r][d0 + c] = src[r][s0 + c], c < w (row-major, leading dimensions ldd / lds)
void copy_cols(int64_t nrows, int w, const double* src, int lds, int s0, double* dst, int ldd, int d0,
               hipStream_t s);

// --- lowrank.hip -------------------------------------------------------------------------
// The passes of the operator A + P S P^T (rbl_set_lowrank).  P: rows x rp row-major on the
// device, rp = lr_padded_width(r) (even: 2, 4, 6, 8, 12, 16, 24 or 32; the columns past r zero;
// 0 for r outside [1, 32]), 16-byte aligned; X, U: rows x b
// row-major blocks, 1 <= b <= RBL_MAX_BLOCK; w, c: rp x b row-major; S: r x r row-major.
// Fixed summation orders, no atomics; 16-byte accesses when b is even and the block is 16-byte
// aligned, else 8-byte.
//   lr_project: w = P^T X; part holds lr_project_grid(rows, b, rp) x rp x b doubles (the
//               per-workgroup partials, added by reduce_slab);
//   lr_small:   c = S w (the rows r <= i < rp of c zero), one workgroup;
//   lr_update:  U[row][:] += P[row][:] c for row < rows — rows past `rows` are not touched.
int lr_padded_width(int r);
int lr_project_grid(int64_t rows, int b, int rp);
void lr_project(int64_t rows, int b, int rp, const double* P, const double* X, double* part,
                double* w, hipStream_t s);
void lr_small(int r, int rp, int b, const double* S, const double* w, double* c, hipStream_t s);
void lr_update(int64_t rows, int b, int rp, const double* P, const double* c, double* U,
               hipStream_t s);

// --- cg.hip: the row passes of the batched preconditioned CG solver (rbl_solve) -------------------
// X, R, P, W, B: n x b row-major blocks, 1 <= b <= RBL_MAX_BLOCK; part holds cg_grid(nrows, b) x 2 b
// doubles (the workgroup partials of a pass, added into `dots` by reduce_slab).  Fixed summation
// orders, no atomics; 16-byte accesses when b is even and every block is 16-byte aligned.
// The per-column scalars, b entries each, on the device.  status: kCgActive while the column
// iterates, then kCgConverged or kCgNotPosDef (a frozen column: its x, r, p are not stored again).
// hist (null: none): (alpha_j, beta_j) of iteration j at hist[(2 j + {0, 1}) * b + column].
constexpr int kCgActive = -1, kCgConverged = 0, kCgNotPosDef = 2;
struct CgScalars {
  double* rho = nullptr;
  double* alpha = nullptr;
  double* beta = nullptr;
  double* bb = nullptr;   // |b|^2
  double* rr = nullptr;   // |r|^2 of the recurrence
  int* iters = nullptr;
  int* status = nullptr;
  int* nactive = nullptr;  // one int: the columns still active after the last cg_beta
  double* hist = nullptr;
};
int cg_grid(int64_t nrows, int b);
//   cg_resid:  R = B - (W + sigma X) (X null: R = B; W, X not read), dots = [|b|^2 (b), |r|^2 (b)];
//   cg_dot:    dots[c] = p_c^T (w_c + sigma p_c);
//   cg_alpha:  alpha = rho / pap (one workgroup); 0 for a frozen column; pap <= 0 or not finite
//              freezes the column as kCgNotPosDef;
//   cg_update: x += alpha p, r -= alpha (w + sigma p) on the active columns, dots[c] = |r_c|^2;
//   cg_small:  c = diag(dv) w (w, c: rp x b row-major; dv: rp entries);
//   cg_beta:   rho' = |r|^2 + w^T c (rp > 0; w = V^T r, c = dv o w), beta = rho' / rho, the iteration
//              counted, (alpha, beta) appended to hist at `iter`, the column frozen as kCgConverged
//              once |r|^2 <= tol2 |b|^2, *nactive counted (one workgroup).  init: dots is cg_resid's,
//              the scalars are set up (iters = 0, beta = 0) and nothing is appended;
//   cg_dir:    p = r + V c + beta p on the active columns (rp = 0: p = r + beta p; else V: nrows x rp
//              row-major, rp = lr_padded_width(r), as lr_update's P).
void cg_resid(int64_t nrows, int b, const double* B, const double* W, const double* X, double sigma,
              double* R, double* part, double* dots, hipStream_t s);
void cg_dot(int64_t nrows, int b, const double* P, const double* W, double sigma, double* part,
            double* dots, hipStream_t s);
void cg_alpha(int b, const double* pap, const CgScalars& sc, hipStream_t s);
void cg_update(int64_t nrows, int b, double* X, double* R, const double* P, const double* W, double sigma,
               const CgScalars& sc, double* part, double* dots, hipStream_t s);
void cg_small(int rp, int b, const double* dv, const double* w, double* c, hipStream_t s);
void cg_beta(int b, int rp, bool init, int iter, const double* dots, const double* w, const double* c,
             double tol2, const CgScalars& sc, hipStream_t s);
void cg_dir(int64_t nrows, int b, int rp, const double* R, double* P, const double* V, const double* c,
            const CgScalars& sc, hipStream_t s);

// --- kernelop.hip: the implicit kernel matrix (rbl_set_matrix_kernel) ---------------------------
// Op = diag(scale) K diag(scale) + nugget I, K_ij = kappa(x_i, x_j) over the n points X (device,
// row-major n x d4, d4 = 4 ceil(d / 4) <= kKernMaxDim, the columns past d zero; nrm[i] = |x_i|^2
// from kernop_norms).  scale null: all ones.  kind: kKernRbf exp(-gamma |x-y|^2), kKernLaplace
// exp(-gamma |x-y|), kKernPoly (gamma x.y + coef0)^degree (the values of RBL_KERNEL_*).
constexpr int kKernRbf = 0, kKernLaplace = 1, kKernPoly = 2;
constexpr int kKernMaxDim = 256;
struct KernOp {
  int64_t n = 0;
  int d4 = 0;
  int kind = kKernRbf;
  int degree = 1;
  double gamma = 1.0, coef0 = 0.0, nugget = 0.0;
  const double* X = nullptr;
  const double* nrm = nullptr;
  const double* scale = nullptr;
};
void kernop_norms(int64_t n, int d4, const double* X, double* nrm, hipStream_t s);
// U = Op Q for row-major n x b blocks (U must not alias Q), any b >= 1: column chunks of 32 and 16
// on fp64 MFMA, the rest in chunks of <= 8 by the plain kernel.  Rows past n are not touched.
// Fixed summation order, no atomics, no scratch.  false: bad shape (nothing launched).
bool kernop_apply(const KernOp& op, const double* Q, int b, double* U, hipStream_t s);

// --- kernelop_cross.hip: the rectangular cross-kernel product (rbl_kernel_cross) ------------------
// Y = diag(sr) kappa(R, C) diag(sc) W: R mr x d4 row points, C mc x d4 column points (both as X
// above, norms from kernop_norms), W mc x b and Y mr x b row-major with leading dimension b.  sr / sc
// null: all ones.  No diagonal rule and no nugget.
struct KernCross {
  int64_t mr = 0, mc = 0;
  int d4 = 0;
  int kind = kKernRbf;
  int degree = 1;
  double gamma = 1.0, coef0 = 0.0;
  const double* R = nullptr;
  const double* rnrm = nullptr;
  const double* C = nullptr;
  const double* cnrm = nullptr;
  const double* sr = nullptr;
  const double* sc = nullptr;
};
// The split of the column range, a function of the shapes alone (never of the device, so the bits do
// not depend on the CU count): the fewest splits that bring ceil(mr / 64) x S to kKernCrossWorkgroups
// workgroups, at most kKernCrossMaxSplits, and no split shorter than kKernCrossMinStages stages of
// kern_jt column points (so never more splits than stages); 1 when the rows alone reach the target.
constexpr int kKernCrossWorkgroups = 512, kKernCrossMaxSplits = 64, kKernCrossMinStages = 4;
int kernop_cross_splits(int64_t mr, int64_t mc, int d4);
// Any b >= 1 on fp64 MFMA (column chunks of 32, 16 and a zero-padded last chunk).  splits = 1: the
// main kernel writes Y, part is not used.  splits > 1 (<= kKernCrossMaxSplits and <= the stages of
// the column range): part holds splits x mr x b doubles; the partials are added in ascending split
// order by one owner thread per output.  Fixed summation order, no atomics.  false: bad shape
// (nothing launched).
bool kernop_cross(const KernCross& op, const double* W, int b, double* Y, double* part, int splits,
                  hipStream_t s);

// --- kernelop_knn.hip: k nearest column points of every row point (rbl_kernel_knn) ----------------
// R mr x d4 row points and C mc x d4 column points with their norms, as KernCross holds them.  Row i
// gets the k smallest (d2, j) over the column points j, d2 = max((|r_i|^2 + |c_j|^2) - 2 r_i.c_j, 0)
// from the cross product's MFMA chain, the smaller index first on equal d2; `self`: R and C are one
// array (mr == mc) and the pair (i, i) is skipped by index.  1 <= k <= kKernKnnMax, k <= mc (mc - 1
// with self).
constexpr int kKernKnnMax = 64;
struct KernKnn {
  int64_t mr = 0, mc = 0;
  int d4 = 0;
  int k = 0;
  bool self = false;
  const double* R = nullptr;
  const double* rnrm = nullptr;
  const double* C = nullptr;
  const double* cnrm = nullptr;
};
// idx and d2: mr x k row-major, each row sorted ascending in (d2, j).  splits as kernop_cross
// (kernop_cross_splits is the rule): with splits > 1, part_idx and part_d2 hold splits x mr x k
// entries and one thread per row merges the splits' lists.  The answer is unique — it does not depend
// on splits — and there are no atomics.  false: bad shape (nothing launched).
bool kernop_knn(const KernKnn& op, int32_t* idx, double* d2, int32_t* part_idx, double* part_d2, int splits,
                hipStream_t s);
#ifdef RBL_KNN_COUNT
// diagnostics build: {pair tiles a wave computed, those on which a lane inserted} since the last reset
bool kernop_knn_counts(unsigned long long out[2], bool reset);
#endif

// --- pchol.hip: partial pivoted Cholesky of the kernel matrix (rbl_kernel_pchol) ------------------
// L L^T ~ diag(scale) K diag(scale) over the points of op (its nugget does not enter), at most R <=
// min(n, kPcholMaxRank) greedy steps, n <= 2^31 - 65.  Every buffer on the device:
//   L       ldl x R doubles, column-major, ldl >= n (zeroed by the run; columns past the rank stay 0)
//   d       n doubles, the residual diagonal
//   pmax, ptrace, pidx   2 pchol_slabs(n) entries each: the workgroups' partials, two buffers
//   piv     R int32 (-1 past the rank), trace R + 1 doubles (0 past the rank: the caller repeats the last)
//   floor_  1 double, rank 1 int32, flag R + 2 int32 (one stop flag per launch)
constexpr int kPcholMaxRank = 256;
constexpr int kPcholSlabRows = 256;
static_assert(kPcholMaxRank <= kPcholSlabRows, "one thread per earlier column stages L[p, 0..j)");
struct PcholWork {
  double* L = nullptr;
  int64_t ldl = 0;
  double* d = nullptr;
  double* pmax = nullptr;
  double* ptrace = nullptr;
  int32_t* pidx = nullptr;
  int32_t* piv = nullptr;
  double* trace = nullptr;
  double* floor_ = nullptr;
  int32_t* rank = nullptr;
  int32_t* flag = nullptr;
};
int pchol_slabs(int64_t n);  // ceil(n / kPcholSlabRows): a function of n alone
// Enqueues the clears, one init launch and R + 1 step launches on s, nothing read back: stop at step j
// (rank = j) when j == R, !(d_p > 4 (R + 2) 2^-53 dmax0) or trace_j <= tol trace_0.  Fixed summation
// orders, no atomics, no grid-wide synchronisation.  Each workgroup reads all pchol_slabs(n) partials per
// step (one reduction level): meant for n up to ~10^6.  false: bad shape or a NULL buffer (nothing launched).
bool kernop_pchol(const KernOp& op, int R, double tol, const PcholWork& W, hipStream_t s);

// --- kmeans.hip: Lloyd's k-means and k-means++ seeding (rbl_kmeans_run, rbl_kmeans_seed) ----------
// The points as KernOp holds them (row-major n x d4, zero-padded columns, norms from kernop_norms),
// n < 2^31 - 64; the centres c x d4 alike, 1 <= c <= kKmeansMaxClusters.
constexpr int kKmeansMaxClusters = 256;
struct KmeansPoints {
  int64_t n = 0;
  int d4 = 0;
  const double* X = nullptr;
  const double* nrm = nullptr;
};
// The summation geometry of the update, a function of (n, d4, c) alone: `slabs` row slabs of rows_per
// rows, each walked by `rl` row lanes (contiguous sub-slabs, ascending rows), the centres in `tiles`
// tiles of cw (a row is read by the tile of its label only); the record of a slab and of the whole is
// len = c d4 + c + 2 doubles: the sums row-major, the counts, the inertia, the changed labels.
struct KmeansGeometry {
  int slabs = 1, rl = 1, cw = 1, tiles = 1, lds_bytes = 0;
  int64_t rows_per = 0, len = 0;
};
KmeansGeometry kmeans_geometry(int64_t n, int d4, int c);
// label_i = the j with the smallest (d2(i, j), j), d2 = max((|x_i|^2 + |c_j|^2) - 2 x_i.c_j, 0) from
// the MFMA chain of kernop_knn; dmin_i = d2(i, label_i).  label may be null.  No atomics; the answer
// does not depend on the grid.  false: bad shape (nothing launched).
bool kmeans_assign(const KmeansPoints& P, int c, const double* C, const double* cnrm, int32_t* label, double* dmin,
                   hipStream_t s);
// tot (len doubles) <- the record of the labels: part holds slabs x len doubles.  `changed` counts
// label_i != prev_i.  Fixed order, no atomics.
bool kmeans_update(const KmeansPoints& P, int c, const int32_t* label, const int32_t* prev, const double* dmin,
                   double* part, double* tot, hipStream_t s);
// Cnew_j = sum_j / count_j (Cold_j where count_j = 0) with its norms; rec = {inertia, changed,
// |Cnew - Cold|_F^2} (3 doubles)
void kmeans_form(int c, int d4, const double* tot, const double* Cold, double* Cnew, double* cnrm_new, double* rec,
                 hipStream_t s);
void kmeans_fill_labels(int64_t n, int32_t v, int32_t* label, hipStream_t s);
// Seeding round r >= 1 after the pick `last` of round r - 1: w_i <- min(w_i, d2(i, last)) (r = 1: the
// distance itself), 0 at `last`; picked[r] <- the smallest i whose inclusive prefix sum of w exceeds
// u total (total = 0: the smallest index not in picked[0 .. r)).  dnew and w: n doubles; slabtot:
// kmeans_seed_slabs(n) doubles.
int64_t kmeans_seed_slabs(int64_t n);
bool kmeans_seed_round(const KmeansPoints& P, int r, int64_t last, double u, double* dnew, double* w,
                       double* slabtot, int32_t* picked, hipStream_t s);

// --- kernelop_hadamard.hip: kernel-matrix derivative products (rbl_kernel_hadamard) ---------------
// U = (Phi o A B^T) Q over the points of op (its scale and nugget do not enter): Phi_ij = kappa or one
// of its derivatives (the values of RBL_KWEIGHT_*; kernelop_dev.hpp phi), Ap and Bp the n x r factors
// row-major and zero-padded to r4 = 4 ceil(r / 4) columns, Q and U n x b row-major with leading
// dimension b (U must not alias Q).  d4 + r4 <= kKernMaxDim.  Any b >= 1 on fp64 MFMA, one launch
// per column chunk, grid ceil(n / 64), the column range not split; fixed summation order, no atomics,
// no scratch.  false: bad shape or mode (nothing launched).
constexpr int kKernWeightValue = 0, kKernWeightDgamma = 1, kKernWeightDscale = 2;
bool kernop_hadamard(const KernOp& op, int mode, int r4, const double* Ap, const double* Bp, const double* Q,
                     int b, double* U, hipStream_t s);

// --- tsmm.hip ----------------------------------------------------------------------------
// Partial Gram: slab[s][a][c] = sum over rows of split s of W[r][a] * X[r][c]
//   W: run of nW panels (a in [0, nW*w)), X: panels (c in [0, X.count*X.w)).
// Returns the number of splits used; slab must hold splits * (nW*w) * (X.count*X.w).
int gram_splits(int64_t nrows, int nW, int w, int xcols);
void gram_partial(int64_t nrows, const PanelRun& W, const Panels& X, double* slab, int splits,
                  const int* skip, hipStream_t s);
// out[e] = sum_s slab[s][e], e < len.
void reduce_slab(const double* slab, int splits, int64_t len, double* out, const int* skip,
                 hipStream_t s);
// The same for tens of thousands of splits: a two-level sum whose first level writes
// reduce_scratch_splits(splits) x len doubles right after the partials (reserve them).
int reduce_scratch_splits(int splits);
void reduce_slab_many(double* slab, int splits, int64_t len, double* out, hipStream_t s);
// Y = beta*Y + alpha * X * C, X a run of panels (k = nX*X.w), C row-major k x (Y.count*Y.w)
// with leading dimension ldc.  Y may alias X's panels row-for-row (in-place apply).
void tsmm(int64_t nrows, const PanelRun& X, const double* C, int ldc, const Panels& Y,
          double alpha, double beta, const int* skip, hipStream_t s, double* xslab = nullptr,
          int* xgrid = nullptr);

// --- compress.hip: in-place basis compression (rbl_thick_restart) --------------------------
// Panels 0 .. p / X.w - 1 of the run X (m = X.count panels) <- [X_0 .. X_{m-1}] S_dev, with S_dev
// (m X.w) x p row-major on the device, p a multiple of X.w, X.w <= p <= kCompressMaxCols and
// p / X.w <= m.  In place: a workgroup owns whole rows and finishes every load of them before its
// first store (a workgroup barrier between), so no scratch of size n is needed.  X.w in {16, 32}
// runs on fp64 MFMA with the accumulators of all p columns of a 64-row tile in registers (each
// basis element read from HBM once); any other width, or `generic`, takes one thread per output
// column.  Ascending-k sums, no atomics: the same bits on every call.  false: shape not served
// (nothing launched).  kCompressMaxCols is RBL_COMPRESS_MAX_COLS: 64 rows x 512 columns are 128
// fp64 accumulators per lane, half the 512 registers of a lane at one wave per SIMD.
constexpr int kCompressMaxCols = 512;
bool basis_compress_fast(const PanelRun& X, int p);
bool basis_compress(int64_t nrows, const PanelRun& X, const double* S_dev, int p, hipStream_t s,
                    bool generic = false);

// --- reorth.hip: v_mfma_f64_4x4x4f64 fast paths (panel widths 16 / 32), selected by
// gram_splits / gram_partial / tsmm above when applicable.
bool gram44_ok(int64_t nrows, int nW, int w, int xcount, int xw);
int gram44_splits(int64_t nrows, int nW, int w = 32);
void gram44_partial(int64_t nrows, const PanelRun& W, const Panels& X, double* slab, int splits,
                    const int* skip, hipStream_t s);
bool tsmm44_ok(int xw, int ky, int yw);
// Y = beta Y + alpha X C with X fp32 panels (X.base32), widened to fp64 as loaded: the Ritz
// projection over the fp32 basis in one pass (fp64 S and V).  Same shape limits as tsmm44.
void tsmm44_f32x(int64_t nrows, const PanelRun& X, const double* C, int ldc, const Panels& Y,
                 double alpha, double beta, hipStream_t s);
// xslab (optional, Y = [Q_i, Q_{i-1}] of width w = 16 or 32 on the fast path): also the
// partials of Q_{i-1}^T Q_i, *xgrid = tsmm44_xg_grid(nrows) blocks of w x w in xslab (one per
// 128-row tile; reduce_slab over *xgrid); *xgrid = 0 when this form does not apply.
int tsmm44_xg_grid(int64_t nrows);
void tsmm44(int64_t nrows, const PanelRun& X, const double* C, int ldc, const Panels& Y,
            double alpha, double beta, const int* skip, hipStream_t s, double* xslab = nullptr,
            int* xgrid = nullptr);
// [Y0 | Y1] -= X C with both factors rounded to fp32, each split into three bf16 pieces, and six
// piece products per k summed in fp32 on bf16 MFMA (k_tsmm44x32): X fp64 panels of 32, Y two fp64
// panels of 32, C fp64 row-major; for coefficients C of rounding size only (upd32_gate).
// tsmm44x32_ok: the shapes it takes (nrows >= 32, no aliasing).  Cp: workspace of
// tsmm44x32_cpieces(K) 16-bit units (K = 32 X.count), 16-B aligned: the split image of C, written
// by a small kernel ahead of the update on the same stream.
bool tsmm44x32_ok(int64_t nrows, const PanelRun& X, const Panels& Y);
int64_t tsmm44x32_cpieces(int K);
void tsmm44x32(int64_t nrows, const PanelRun& X, const double* C, int ldc, const Panels& Y,
               const int* skip, unsigned short* Cp, hipStream_t s);
// The same update with an fp32 shadow of X (RBL_OPT_UPD32_SHADOW): S holds X.count slots of
// tsmm44x32_shadow_slot(nrows) floats in the kernel's own layout; the leading nsh panels are read
// from S, the others from X as above and their rounded values stored to S — also when *skip is set,
// where no product is formed and Y stays.  Y has the bits of tsmm44x32.  cnt[0] += panels read from
// S, cnt[1] += panels stored to it (device counters).  shadow_block_rowmajor: one slot (host copy)
// as nrows x 32 row-major.
int64_t tsmm44x32_shadow_slot(int64_t nrows);
void tsmm44x32_shadow(int64_t nrows, const PanelRun& X, const double* C, int ldc, const Panels& Y,
                      const int* skip, float* S, int nsh, int* cnt, unsigned short* Cp, hipStream_t s);
void shadow_block_rowmajor(const float* slot, int64_t nrows, float* out);

// --- reorth32.hip: the fp32 Krylov basis (mixed precision, b in {16, 32}) ---------------
// Gram partials slab[s][a][c] = sum over split s of W[r][a] X[r][c] (W: nW fp32 panels of
// width w at Wb + j*wstride, X: xcount fp32 panels of width w), fp32 MFMA per split.
int gram32_splits(int64_t nrows);
void gram32_partial(int64_t nrows, const float* Wb, int64_t wstride, int nW, int w, const float* X0,
                    const float* X1, int xcount, double* slab, int splits, hipStream_t s);
// Y = beta Y + alpha X C: X nX fp32 panels (k = nX*w), C fp64 row-major (rounded to f32),
// Y ycount fp32 panels of width w (Y may alias X's panels row-for-row).
void tsmm32(int64_t nrows, const float* Xb, int64_t xstride, int nX, int w, const double* C, int ldc,
            float* Y0, float* Y1, int ycount, float alpha, float beta, hipStream_t s);
void cvt_f32_to_f64(const float* src, double* dst, int64_t n, hipStream_t s);
void cvt_f64_to_f32(const double* src, float* dst, int64_t n, hipStream_t s);

// --- smallmat.hip ------------------------------------------------------------------------
// Cholesky step of (shifted) CholQR on the b x b Gram G (row-major, symmetric):
//   mode 0: first pass — try unshifted; on breakdown or estimated cond > 3e7 use the
//           Fukaya shift and set need3[0] = 1, need3[1] = 0 (so a third pass runs;
//           need3[1] is the `skip` word of the third pass' kernels);
//   mode 1: later pass — unshifted (falls back to shift if it still breaks).
// Writes R (upper), Rinv, and Rtot = R * Rtot_prev (first pass: Rtot = R).
// If *skip != 0 the kernel does nothing (used for the conditional third pass).
// scratch: 2 b^2 doubles (used only for b > 64: the factor and R^-1 do not fit in LDS there)
void chol_step(const double* G, int b, int64_t nglobal, int mode, double* R, double* Rinv,
               double* Rtot, int* need3, int* status, const int* skip, hipStream_t s,
               double* scratch);
// dst = src (len doubles): B_i stashed for the next step's epilogue, and the out-of-place
// CholQR applies at b > 64; nothing when *skip != 0.
void copy_small(const double* src, double* dst, int64_t len, hipStream_t s, const int* skip = nullptr);
// C = C Rinv (b x b, Rinv upper triangular) unless *skip (k_cloc_rinv)
void cloc_rinv(double* C, const double* Rinv, int b, const int* skip, hipStream_t s);
// C = (C R1inv) R2inv, both upper triangular, b <= 32 (k_cloc_rinv2)
void cloc_rinv2(double* C, const double* R1inv, const double* R2inv, int b, hipStream_t s);
// gate[0] = 1 iff (Q^T U) R^-1 is as good as the Gram Q^T (U R^-1) to eps tau: *need3 == 0 and
// max_c sum_j |R[:, j]| |Rinv[j][c]| <= tau; gate[1] = !gate[0].  b <= 32 (k_cloc_gate)
void cloc_gate(const double* R, const double* Rinv, int b, const int* need3, double tau, int* gate,
               hipStream_t s);
// May the update Y -= W C run with W C formed in fp32 (tsmm44x32)?  C: K x ncols row-major, equal
// on every rank (all-reduced).  g = max_c |C_c|_2 sqrt(K) 2^-24 / eps is the fp32 rounding of a
// column of W C in units of the fp64 rounding of Y; taken iff g <= tau or force (a NaN refuses).
// flags = [skip of the fp32 kernel, skip of the fp64 kernel, taken count, refused count];
// *g_out = g (diagnostics).  ncols <= 64 (k_upd32_gate)
void upd32_gate(const double* C, int K, int ncols, double tau, int force, int* flags, double* g_out,
                hipStream_t s);
// G -= Cm^T Ci with D = [Ci | Cm] (nW b x 2b row-major), b <= 256; a fixed summation order
// (k_cloc_sub)
void cloc_sub(double* G, const double* D, int nW, int b, hipStream_t s);
// dst = src^T (b x b row-major).
void transpose_small(const double* src, double* dst, int b, hipStream_t s);
// stash = [A_i (b x b) | R_tot (b x b) | 4 int flags], Bprev = R_tot, flags cleared (k_stash)
void stash_step(const double* Ai, const double* Rtot, double* Bprev, int* flags, double* stash,
                int b, hipStream_t s);

// --- gen_rmat.hip (R-MAT generator) -------------------------------------
struct RmatParams {
  int64_t n = 0;
  int scale = 0;
  int64_t edges = 0;
  double a = 0.57, b = 0.19, c = 0.19;
  uint64_t seed = 0;
  // RBL_OPT_RELABEL: the matrix is P A P^T, vertex v stored as row / column perm(v) (a seeded
  // Feistel bijection, make_scatter(n, seed ^ kRelabelK)); values and the planted diagonal
  // stay those of the original ids, so the spectrum is A's
  bool relabel = false;
  Scatter perm;
};
constexpr uint64_t kRelabelK = 0x52454C4142454C31ull;  // "RELABEL1"
// deg[r] += 1 per kept draw endpoint (duplicates counted; zero-filled deg of n int32)
void rmat_degree(const RmatParams& p, int32_t* deg, hipStream_t s);
// local CSR of rows [r0, r1): rowptr_dev (m+1, caller-allocated), col/val allocated here (with
// kCsrPad zero entries); max_keys >= the own rows' kept draw endpoints.  0 or a negative status.
int rmat_local_csr(const RmatParams& p, int64_t r0, int64_t r1, int64_t max_keys, int nplant,
                   const double* plant_dev, int64_t* rowptr_dev, int32_t** col_dev,
                   double** val_dev, int64_t* nnz_out, hipStream_t s);
// per-rank column footprint of a local CSR: lo[q] = min, hi[q] = max + 1 (atomics; lo/hi
// initialised to ~0 / 0), bounds_dev = the P+1 row boundaries
void col_footprint(const int32_t* col, int64_t nnz, const int64_t* bounds_dev, int P,
                   unsigned long long* lo, unsigned long long* hi, hipStream_t s);

// --- gen.hip ---------------------------------------------------------------------------
// Hash-window matrix rows [r0,r1): counts per row, then fill given rowptr (0-based, local).
// circuit-like matrix (gen.hip; oracle/matgen.py circuit_like_csr): rows [r0, r1) of the
// scattered index space, counts then CSR fill (columns sorted)
void circ_count(int64_t n, int64_t width, double p, uint64_t seed, int64_t r0, int64_t r1,
                int32_t* counts, hipStream_t s);
void circ_fill(int64_t n, int64_t width, double p, uint64_t seed, int64_t r0, int64_t r1,
               const int64_t* rowptr, int nplant, const double* plant_dev, int32_t* col,
               double* val, hipStream_t s);
// indexed halo (several ranks, unbanded A): out[i] = Q[idx[i]] (rows of b doubles); mark[c] = 1
// for every column c outside [r0, r1); col[k] = map[col[k]]
void gather_rows(const double* Q, const int32_t* idx, int64_t nrows, int b, double* out,
                 hipStream_t s);
void mark_cols(const int32_t* col, int64_t nnz, int64_t r0, int64_t r1, uint8_t* mark,
               hipStream_t s);
void remap_cols(int32_t* col, int64_t nnz, const int32_t* map, hipStream_t s);
void hw_count(int64_t n, int64_t W, double p, uint64_t seed, int64_t r0, int64_t r1,
              int32_t* counts, hipStream_t s);
void hw_fill(int64_t n, int64_t W, double p, uint64_t seed, int64_t r0, int64_t r1,
             const int64_t* rowptr, int nplant, const double* plant_dev, int32_t* col,
             double* val, hipStream_t s);
// N(0,1) block, row-major n_local x b, global row offset r0, counter-based from seed.
// N(0,1) start block of global rows r0.. (row r drawn from its id; with `perm` (the relabel of
// the matrix, RBL_OPT_RELABEL) from its original id perm^-1(r), so a relabelled run starts
// from the same block as the plain one, its rows permuted)
void randn_block(double* Q, int64_t nrows, int b, int64_t r0, uint64_t seed, hipStream_t s,
                 const Scatter* perm = nullptr);
// Per-tile column range of the CSR (tile = `tile_rows` rows), for the LDS-window SpMM.
void tile_col_range(const CsrDev& A, int tile_rows, int64_t* cmin, int64_t* cmax, hipStream_t s);
// column-major (ld = nrows) <-> row-major (ld = w) transposes for the boundary
void colmajor_to_rowmajor(const double* src, int64_t nrows, int w, double* dst, hipStream_t s);
void rowmajor_to_colmajor(const double* src, int64_t nrows, int w, double* dst, hipStream_t s);

}  // namespace rbl
