// rbl_api.cpp — the C-ABI of librbl_hip.so (include/rbl_hip.h).
//
// Host orchestration of one block Lanczos step on one GPU (or one rank of a row-partitioned
// job).  Mirrors the device part of Julia/RBL_gpu.jl:134-203; the CPU part (T_j band,
// dsbev, sort, convergence — Julia/common.jl) stays with the caller.
//
// HBM plan: A (CSR, int64 rowptr / int32 col / fp64 val), the WHOLE Krylov basis
// (max_blocks+1 slots of n_local x b, row-major), U, one scratch block, the Gram slab and
// b x b scalars.  Nothing but b x b blocks crosses PCIe per step.
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rbl_hip.h"
#include "comm.hpp"
#include "kernels.hpp"

using namespace rbl;

// Every device or pinned-host buffer is a DevBuf / PinBuf declared in the struct of its lifetime
// (MatrixBufs, RunBufs, CtxBufs) and nowhere else: free_matrix and free_run assign an empty struct,
// so a buffer declared there is released with its lifetime and on every error path.
namespace rbl::api {

// Owner of one device allocation of `count` T: move-only, released by the destructor, by reset()
// and by a move assigned over it.  Converts to T*, so it is used where the raw pointer was.
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  void adopt(T* q) {  // takes over an allocation a kernels.hpp routine handed out
    reset();
    p = q;
  }
  operator T*() const { return p; }
};

// The pinned-host twin (hipHostMalloc with `flags` / hipHostFree).
template <class T>
struct PinBuf {
  T* p = nullptr;
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { reset(); }
  hipError_t alloc(size_t count, unsigned flags) {
    reset();
    const hipError_t e = hipHostMalloc(&p, count * sizeof(T), flags);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
  }
  operator T*() const { return p; }
};

// A CSR of some rows with the task table of its segmented gather (build_seg): a column tier
// (CsrDev::seg_tier), the push tier, one orientation of a rectangular B
struct SegTierBuf {
  DevBuf<int64_t> rowptr;
  DevBuf<int32_t> col;
  DevBuf<double> val;
  int64_t ntasks = 0, nlong = 0;
  DevBuf<int64_t> trow;
  DevBuf<int32_t> tinfo;
  DevBuf<int64_t> slot_k0;
  DevBuf<int64_t> lrow;
  DevBuf<int64_t> lslot;
  DevBuf<double> scratch;
};

// ---- buffers that live as long as the matrix (free_matrix); the parts that are also released
// ---- alone are structs of their own

// column-panel SpMM (spmm_panel.hip; free_panels): per 256-row block its first and last 256-row
// Q panel
struct PanelBufs {
  DevBuf<int32_t> d_panel_blk;
  DevBuf<uint16_t> d_panel_cnt;  // per block, panel and row: the row's entries in the panel
  DevBuf<uint32_t> d_panel_st;   // ... and their first record (from the block's base)
  DevBuf<uint8_t> d_panel_col;   // the records panel-major within a block: column in the panel
  DevBuf<double> d_panel_val;    //   and value
};

// segmented-gather task table of the whole CSR (spmm.hip variant 5; CsrDev::seg_*)
struct SegTableBufs {
  DevBuf<int64_t> d_seg_trow;
  DevBuf<int32_t> d_seg_tinfo;
  DevBuf<int64_t> d_seg_slot_k0;
  DevBuf<int64_t> d_seg_lrow;
  DevBuf<int64_t> d_seg_lslot;
  DevBuf<double> d_seg_scratch;
};

// column tiers and the indexed halo (free_tiers)
struct TierBufs {
  // column tiers of the segmented gather (RBL_SEG_TIERS, one rank; CsrDev::seg_tier): each a
  // CSR of the same rows holding the nonzeros of one column-degree tier, with its task table
  SegTierBuf seg_tier[3];
  DevBuf<int32_t> d_send_idx;  // indexed halo: local row ids the peers asked for, grouped by peer
  SegTierBuf push_tier;        // push/pull split: tier 1 transposed (rows = ghost slots)
  DevBuf<int64_t> d_ps_rows;   // own rows that receive partials, ascending
  DevBuf<int64_t> d_ps_ptr;    //   their slots in d_precv (peer order)
  DevBuf<int64_t> d_ps_slot;
};

// rank-one shift C = B - u v^T (rbl_set_rect_shift; free_rect_shift).  d_rect_ts holds t = Q^T v
// and s = Y^T u (rect_ts_cols doubles each), d_rect_part the workgroup partials of their
// reductions; both sized by ensure_rect_y
struct RectShiftBufs {
  DevBuf<double> d_shift_u;  // m
  DevBuf<double> d_shift_v;  // n
  DevBuf<double> d_rect_ts;
  DevBuf<double> d_rect_part;
};

// implicit symmetric low-rank update (rbl_set_lowrank; free_lowrank).  d_lr_P: n_local x lr_rp
// row-major, the columns past lr_r zero (lr_rp = lr_padded_width(lr_r)); d_lr_S: r x r row-major;
// d_lr_wc holds w = P^T X and c = S w (lr_rp x lr_cols each), d_lr_part the workgroup partials
// of w; the last two are sized by ensure_lr_bufs
struct LowrankBufs {
  DevBuf<double> d_lr_P;
  DevBuf<double> d_lr_S;
  DevBuf<double> d_lr_wc;
  DevBuf<double> d_lr_part;
};

// spectral preconditioner of rbl_solve, M^-1 = I + V diag(dv) V^T (rbl_set_precond_lowrank;
// free_precond).  d_pc_V: n_local x pc_rp row-major, the columns past pc_r zero (pc_rp =
// lr_padded_width(pc_r)); d_pc_dv: pc_rp entries, zero past pc_r.  Its own buffers: the operator's
// low-rank update (LowrankBufs) may be set at the same time.
struct PrecondBufs {
  DevBuf<double> d_pc_V;
  DevBuf<double> d_pc_dv;
};

struct MatrixBufs : PanelBufs, SegTableBufs, TierBufs, RectShiftBufs, LowrankBufs, PrecondBufs {
  DevBuf<int64_t> d_rowptr;
  DevBuf<int32_t> d_col;
  DevBuf<double> d_val;
  DevBuf<int64_t> d_tcmin;
  DevBuf<int64_t> d_tcmax;
  DevBuf<int64_t> d_tinfo;
  DevBuf<uint16_t> d_bpos;     // band kernel: per-nonzero dense-tile positions
  DevBuf<double> d_bt;         // band-tile kernel: the CSR in MFMA-ordered 16-row band tiles
  DevBuf<uint64_t> d_btp_hdr;  // the band tiles packed (zeros dropped; replaces d_bt)
  DevBuf<double> d_bth;        // half band tiles (A symmetric; replaces d_bt), and the
  DevBuf<double> d_bte;        //   first (NG-1)/2 local tiles whole
  DevBuf<double> d_btp_val;
  DevBuf<double> d_zrow;       // 32 zeros: band rows the halo does not hold
  // dense A: local rows in 32-column row-major panels, multiplied by tsmm44 against d_qfull
  // (all n rows of Q, zero-padded to 32 * dense_panels rows, b <= 64 columns)
  DevBuf<double> d_dense;
  DevBuf<double> d_qfull;
  // rectangular sparse B: [0] B's rows (column ids), [1] B^T's rows (row ids); Y = B Q_i passes
  // through d_rect_y (m x rect_y_cols)
  SegTierBuf rect_side[2];
  DevBuf<double> d_rect_y;
  // implicit kernel matrix (rbl_set_matrix_kernel; kernelop.hip): the points row-major n x kern_d4
  // (zero-padded columns), their squared norms, and the scale of rbl_set_kernel_scale (null: ones)
  DevBuf<double> d_kern_x;
  DevBuf<double> d_kern_nrm;
  DevBuf<double> d_kern_scale;
};

// ---- buffers that live as long as one Krylov run (free_run)
struct RunBufs {
  DevBuf<double> d_basis;  // (max_blocks+1) slots (fp64 basis)
  // pinned host slots of the spilled blocks (block j at h_spill[j - resident]), pinned when
  // the block is first written out: host memory grows with the blocks a run really spills
  std::vector<PinBuf<char>> h_spill;
  DevBuf<double> d_stage;  // one n_local x b staging block for spilled blocks
  // fp32 basis (mixed precision, RBL_gpu.jl with FLOAT = Float32): slots in d_basis32, the
  // current and previous block widened to fp64 in d_Qi64 / d_Qm64 for A Q, 3-term and QR
  DevBuf<float> d_basis32;
  DevBuf<float> d_stage32;
  DevBuf<double> d_Qi64;
  DevBuf<double> d_Qm64;
  DevBuf<double> d_U;
  DevBuf<double> d_T;        // scratch n_local x max(b,k)
  DevBuf<double> d_qext;     // halo-extended Q_i (multi-rank)
  DevBuf<double> d_sendbuf;  // indexed halo: n_send x b
  DevBuf<double> d_pushbuf;  // n_ghost x b: pushed partial rows
  DevBuf<double> d_precv;    // n_send x b: partial rows received for own rows
  DevBuf<double> d_slab;
  DevBuf<double> d_C;        // Gram result (<= (max_blocks)*b x 2b)
  DevBuf<unsigned short> d_C16;  // b = 32: d_C as the three bf16 images of k_tsmm44x32 (RBL_OPT_UPD32)
  DevBuf<double> d_small;    // R, Rinv, Rtot, Bprev, Ai, G (b x b each)
  DevBuf<int> d_flags;       // [need3, skip3, status0, status1, cloc derived, cloc direct]
  PinBuf<double> h_pin;      // pinned staging: Ai, Rtot (2 b x b)
  PinBuf<double> h_hist;     // rbl_step_async stash: per step i, Ai and Rtot (2 b x b) and the
                             //   step's 4 flags (2 doubles' room): stash_rec(b) doubles each
  DevBuf<double> d_stash;    // the device side of one such record (k_stash; RBL_STASH_COPY=1)
  // locked Ritz vectors of the restarted variants (restarted.jl: Qlock / Qlock_gpu), fp64,
  // vector j at d_lock + j * nloc (a width-1 panel)
  DevBuf<double> d_lock;
  // thick restart: W^T ((kb b) x b row-major) of the pending arrow step, and the compression's S
  // ((m b) x (kb b) row-major).  Both grow on demand and hold nothing of size n.
  DevBuf<double> d_arrow_W;
  DevBuf<double> d_tr_S;
  // Chebyshev filter: the work blocks of the recurrence beside U, each (n_local + kRowPad) x
  // filt_cols and zeroed like every block an SpMM writes (d_filt[2] only while a series is set)
  DevBuf<double> d_filt[3];
  // Rayleigh-Ritz on A between rbl_ritz_project and rbl_ritz_finish: V = [Q_1..Q_m] S and
  // W = A V, (n_local + kRowPad) x ritz_kp row-major (ritz_kp = ritz_k rounded up to even)
  DevBuf<double> d_rv;
  DevBuf<double> d_rw;
  // RBL_OPT_UPD32_SHADOW: (float) of basis blocks 0 .. max_blocks - 3 for the fp32 partial-reorth
  // update, shadow_slot floats each in k_tsmm44x32's own layout; null: no shadow in this plan
  DevBuf<float> d_shadow;
};

// ---- buffers that live as long as the context (rbl_free)
struct CtxBufs {
  PinBuf<char> h_d2h[2];  // pinned slots of the staged D2H (d2h_staged)
  // RBL_OPT_UPD32 (k_upd32_gate); the counts are rbl_path_stats entries, so they outlive a run
  DevBuf<int> d_upd32;       // [skip fp32 kernel, skip fp64 kernel, taken, refused, shadow panels
                             //  read, panels rounded into the shadow]
  DevBuf<double> d_upd32_g;  // the gate's value g of step i at [i % kUpd32Log] (diagnostics)
  // k-means points (rbl_kmeans_set_points; kmeans.hip): row-major km_n x km_d4 (zero-padded columns)
  // and their squared norms.  Independent of the matrix: set_matrix and free_matrix leave them alone.
  DevBuf<double> d_km_x;
  DevBuf<double> d_km_nrm;
};

}  // namespace rbl::api

struct rbl_ctx : rbl::api::MatrixBufs, rbl::api::RunBufs, rbl::api::CtxBufs {
  int device = 0;
  hipStream_t stream = nullptr;
  int nranks = 1, rank = 0;
  rbl::Comm* comm = nullptr;  // RCCL or in-process transport (comm.hpp); null for one rank
  std::string err;

  // matrix (local rows [r0,r1) of an n x n symmetric matrix)
  int64_t n = 0, r0 = 0, r1 = 0, nloc = 0, nnz = 0;
  int64_t panel_nblk = 0;
  int panel_rpg = 4;        // rows per 16-lane group: blocks of 64 panel_rpg rows
  int panel_ch = 48;        // records per row and chunk load
  bool panel_auto = false;  // chosen by default: every staged Q row used >= 4 times on average
  int64_t panel_span = 0;   // the widest block window, Q rows
  int bt_ng = 0;            // the band groups of d_bt (0: not applicable)
  int64_t seg_ntasks = 0, seg_nlong = 0;
  int seg_ntiers = 0;
  bool seg_split = false;             // several ranks: tiers = own / halo columns
  // indexed halo (with seg_split): the halo tier's columns renumbered to ghost slots
  // [0, n_ghost) in d_qext, grouped by owning rank; each step every rank packs the rows its
  // peers asked for (d_send_idx, local row ids grouped by peer) and sends only those
  bool ghost = false;
  int64_t n_ghost = 0, n_send = 0;
  std::vector<int64_t> ghost_cnt, ghost_off, send_cnt, send_off;
  const double* ghost_local = nullptr;  // alias: the block the last exchange sent from
  bool ghost_active = false;          // the last exchange was the indexed one (use_ghost)
  bool halo_overlap = true;           // RBL_OPT_HALO_OVERLAP
  // push/pull split of the indexed halo (RBL_OPT_HALO_PUSH): of every off-rank product
  // A[r,c] Q[c] the rank holding the higher-ranked endpoint ((degree, id) order) does the work —
  // it pulls Q[c] when c ranks higher (tier 1: the ghost slots), and when r ranks higher the
  // owner of c computes A[c,r] Q[c] from its own rows and pushes the partial row r (the push
  // tier, rows = ghost slots of that owner, columns = its own rows); received partials are
  // added to U in peer order (d_ps_*)
  int halo_push_opt = 2;              // 0 off, 1 on, 2 on when it moves fewer rows (default)
  bool push = false;
  int64_t push_rows = 0;              // = n_ghost (rows of the push tier)
  int64_t n_ps_rows = 0;
  size_t push_cap = 0;                // capacity (doubles) of d_pushbuf / d_precv
  int64_t push_pred_rows = 0, pull_pred_rows = 0;  // rows per SpMM, summed over ranks (setup)
  hipEvent_t ev_push_ready = nullptr, ev_push_done = nullptr;
  hipStream_t hstream = nullptr;      // the overlapped halo exchange
  hipEvent_t ev_qready = nullptr, ev_halo = nullptr;
  // dense A (RBL_gpu(A::Matrix{Float64})): panel p = columns [32p, 32p+32), zero past n
  bool dense = false;
  int64_t dense_panels = 0;
  int qfull_cols = 0;         // columns d_qfull was sized for
  // rectangular sparse B, m x n (rbl_set_matrix_normal): both orientations as CSR with their
  // task tables for the gather pair of spmm_rect.hip; the Krylov operator is B^T B on n rows
  bool rect = false;
  int64_t rect_m = 0;
  int rect_y_cols = 0;
  // rank-one shift C = B - u v^T (rbl_set_rect_shift): the operator is then C^T C
  bool rect_shift = false;
  int rect_ts_cols = 0;
  // implicit kernel matrix over n points in kern_d dimensions (rbl_set_matrix_kernel): the operator
  // is diag(s) K diag(s) + kern_nugget I, evaluated by kernelop.hip and never stored
  bool kernop = false;
  int kern_d = 0, kern_d4 = 0, kern_kind = 0, kern_degree = 0;
  double kern_gamma = 0.0, kern_coef0 = 0.0, kern_nugget = 0.0;
  // k-means points (rbl_kmeans_set_points): km_n points in km_d dimensions; km_n = 0: none
  int64_t km_n = 0;
  int km_d = 0, km_d4 = 0;
  // implicit symmetric low-rank update (rbl_set_lowrank): the operator is A + P S P^T, applied
  // by apply_A after the SpMM
  int lr_r = 0, lr_rp = 0;
  int lr_cols = 0;
  // spectral preconditioner of rbl_solve (rbl_set_precond_lowrank): rank and padded width; 0: none
  int pc_r = 0, pc_rp = 0;
  int64_t ntiles = 0, tiles_per_wg = 0;
  bool window_ok16 = false, window_ok32 = false;
  bool band_ok16 = false, band_ok32 = false;
  bool band_gram = false;                 // band kernel may form A_i (tile rows ring-resident)
  bool band_pair = false;                 // band kernel may stage row pairs with one load set
  std::vector<int64_t> bounds;            // nranks+1
  std::vector<int64_t> need_lo, need_hi;  // rows I need from rank q
  std::vector<int64_t> give_lo, give_hi;  // rows rank q needs from me
  int64_t ext_lo = 0, ext_hi = 0;         // global rows held in d_qext
  bool split_halo = true;                 // RBL_OPT_SPLIT_HALO
  bool keep_csr = true;                   // RBL_OPT_KEEP_CSR
  int relabel_opt = 0;                    // RBL_OPT_RELABEL (applies to the next generator call)
  bool relabeled = false;                 // the matrix held is P A P^T (rmat generator)
  rbl::Scatter relabel_perm;              //   with this P: vertex v at row perm(v)
  bool csr_dropped = false;               // values / column ids released (band tiles only)

  // Krylov run
  int b = 0, max_blocks = 0, nblocks = 0;
  int64_t slot = 0;           // nloc * b
  int basis_bits = 64;
  // host spill (RBL_OPT_DEVICE_BLOCKS): blocks j < resident live in d_basis slot j; blocks
  // j >= resident in working slot resident + (j & 1) while among the two newest, and in
  // pinned host slot j - resident once final (copied during step j + 2)
  int dev_blocks_opt = 0;
  bool auto_planned = false;  // the current basis plan came from RBL_OPT_DEVICE_BLOCKS = -1
  int resident = INT32_MAX;
  hipStream_t cstream = nullptr;      // D2H copies of finished spilled blocks
  hipEvent_t ev_fin = nullptr, ev_d2h[2] = {nullptr, nullptr};
  // rbl_step_async: step i's stash (A_i, R_tot, flags) has landed when step_ev[i] completes, so
  // rbl_fetch waits for the steps it returns, not for steps enqueued after them
  std::vector<hipEvent_t> step_ev;
  bool d2h_pending[2] = {false, false};
  int64_t T_cols = 0;
  size_t qext_cap = 0;        // capacity of d_qext in doubles (grown by ensure_qext)
  size_t slab_elems = 0;
  size_t C_elems = 0;
  hipEvent_t ev_d2h_slot[2] = {nullptr, nullptr};
  hipStream_t rstream = nullptr;      // the Ritz row pieces (ritz_pipelined)
  hipEvent_t ev_ritz[9] = {};         // S uploaded, then each row piece finished on rstream
  // k_stash writes the record straight into h_pin / h_hist (coherent pinned memory, these are
  // their device addresses) instead of a device record plus a D2H copy, which the SDMA engine
  // ran ~60-80 us after the kernel, on the step's critical path
  bool stash_direct = true;
  double* dv_pin = nullptr;   // alias: the device address of h_pin
  double* dv_hist = nullptr;  // alias: the device address of h_hist
  bool flags_clean = false;   // d_flags already zero (the last step's k_stash cleared them)
  int fetched = 1;            // steps < fetched have been returned by rbl_fetch
  bool have_bprev = false;
  int nlock = 0, lock_cap = 0;
  // thick restart (rbl_thick_restart): arrow_kb > 0 while the arrow step is pending — the basis is
  // [Y_1 .. Y_kb, Q_{m+1}] and step kb + 1 forms U = Op Q_{m+1} - [Y_1 .. Y_kb] W^T
  int arrow_kb = 0;
  size_t arrow_W_cap = 0, tr_S_cap = 0;
  // Chebyshev filter (rbl_set_filter; degree 0: none): the Krylov operator is p(A), applied by a
  // three-term recurrence through the work blocks d_filt, sized at rbl_start
  int filt_deg = 0;
  double filt_lo = 0.0, filt_hi = 0.0, filt_ref = 0.0;
  int filt_cols = 0;
  // Chebyshev series (rbl_set_filter_series; empty: none): p(A) = sum_j ser_mu[j] T_j((A - c)/e)
  // over [ser_lo, ser_hi]; its recurrence rotates through three work blocks.  At most one of
  // filt_deg > 0 and a series holds.
  std::vector<double> ser_mu;
  double ser_lo = 0.0, ser_hi = 0.0;
  int ritz_k = 0;

  // options
  int timers = 0;  // RBL_OPT_TIMERS: 0 off, 1 every stage, 2 the SpMM and partial-reorth stages
  int reorth_order = 0;
  int spmm_variant = 0;
  int fuse = 7;               // RBL_OPT_FUSE
  // the local-reorth coefficient Q_{i-1}^T Q_i of step cloc_step (S_CLOC), formed by the QR of
  // step cloc_step - 1 or by the last partial-reorth update of step cloc_step; 0: none
  int cloc_step = 0;
  bool cloc_final = false;    // formed after this step's reorth (valid whatever its flags)
  // RBL_OPT_CLOC_DERIVE: S_CLOC from the 3-term pass's M = Q_i^T U' and CholQR's factors, and
  // through a block-CGS partial reorth as G - Cm^T Ci (cloc_derive_on)
  bool cloc_derive = true;
  int cloc_src = 0;           // who formed S_CLOC: 0 a Gram pass, 1 the 3-term pass, 2 G - Cm^T Ci
  // RBL_OPT_UPD32: the partial-reorth update W C on fp32 MFMA where its coefficients are rounding
  // residue (0 off, 1 decided per step on the device by upd32_gate, 2 always: tests and probes)
  int upd32 = 1;
  // RBL_OPT_UPD32_SHADOW: that update reads W from d_shadow.  shadow_valid: the leading slots whose
  // shadow holds (float) of the block as it stands; whoever writes a basis block outside the
  // step's own pattern (slots >= i - 2 in step i) lowers it (shadow_written)
  int shadow_opt = 1;
  int shadow_valid = 0;
  int64_t shadow_slot = 0;  // floats per shadow slot
  size_t shadow_bytes = 0;
  bool plan_all_resident = false;  // this run was started with RBL_OPT_DEVICE_BLOCKS = 0
  std::vector<int> step_flags;  // part_reorth flags per step (the fusion's schedule guess)
  double stage_ms[RBL_NUM_STAGES] = {0};
  // collectives issued by this rank since the last reset (rbl_comm_stats): all-reduce calls and
  // bytes, grouped halo exchanges and the bytes sent / received in them
  int64_t comm_stats[RBL_COMM_NSTATS] = {0};
  // time spent in this rank's collectives since the last rbl_comm_stats reset
  // (RBL_COMM_*_HOST_NS / *_DEV_NS): host wall time inside the transport call, and the
  // hipEvent span of the call on its stream (recorded while RBL_OPT_TIMERS is 1)
  int64_t comm_host_ns[2] = {0, 0};  // [0] all-reduces, [1] halo exchanges
  double comm_dev_ms[2] = {0.0, 0.0};
  // which code path each step took (rbl_path_stats): counted on the host as the work is issued,
  // so a test can assert the path itself instead of timing it
  int64_t path_stats[RBL_PATH_NSTATS] = {0};
  // parent: the stage whose span encloses this one on the same stream (a collective inside
  // "3-term" / "qr" / "part reorth"), whose time excludes it; -1 none
  struct Mark { int stage; hipEvent_t a, b; int parent = -1; };
  std::vector<Mark> marks;
  struct OpenStage { int stage; hipStream_t st; };
  std::vector<OpenStage> open_stages;  // StageScopes alive now, innermost last
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
};

using namespace rbl::api;

namespace {

const char* kStageNames[RBL_NUM_STAGES] = {"AQ", "3-term", "qr", "part reorth", "loc reorth",
                                           "Ritz vectors", "comm", "spill wait"};

int fail(rbl_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}


#define HIPC(expr)                                                                    \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return fail(ctx, _e == hipErrorOutOfMemory ? RBL_ERR_OOM : RBL_ERR_HIP,          \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                 \
  } while (0)
#define COMMC(expr)               \
  do {                            \
    int _s = (expr);              \
    if (_s < 0) return _s;        \
  } while (0)
#define CHK(expr)             \
  do {                        \
    int _s = (expr);          \
    if (_s < 0) return _s;    \
  } while (0)

// device location of fp64 block j: resident slot, or (spilled region) its working slot —
// valid only while j is one of the two newest blocks
double* slotp(rbl_ctx* ctx, int j) {
  const int s = j < ctx->resident ? j : ctx->resident + (j & 1);
  return ctx->d_basis + (int64_t)s * ctx->slot;
}
bool spilled(const rbl_ctx* ctx) { return ctx->resident != INT32_MAX; }
// basis slots >= lowest are (about to be) written: their shadow no longer holds (float) of them
void shadow_written(rbl_ctx* ctx, int lowest) { ctx->shadow_valid = std::min(ctx->shadow_valid, std::max(lowest, 0)); }
// fp64 block j on the device: in place when resident or among the newest two of `nblocks`,
// else copied from pinned host memory into the staging block (on the compute stream)
const double* block_dev(rbl_ctx* ctx, int j, int nblocks, int* st) {
  *st = 0;
  if (j < ctx->resident || j >= nblocks - 2) return slotp(ctx, j);
  const hipError_t e = hipMemcpyAsync(ctx->d_stage, ctx->h_spill[j - ctx->resident],
                                      ctx->slot * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) *st = RBL_ERR_HIP;
  return ctx->d_stage;
}
// fp32 basis: the same slot plan as slotp / block_dev
// pin the host slot of spilled block j on first use (non-coherent pages: the DMA engines
// stream them at PCIe rate both ways)
int spill_slot(rbl_ctx* ctx, int j, size_t elem) {
  auto& h = ctx->h_spill[j - ctx->resident];
  if (!h) {
    const hipError_t e = h.alloc((size_t)ctx->slot * elem, hipHostMallocNonCoherent);
    if (e != hipSuccess) {
      return fail(ctx, e == hipErrorOutOfMemory ? RBL_ERR_OOM : RBL_ERR_HIP,
                  std::string("host spill: hipHostMalloc: ") + hipGetErrorString(e));
    }
  }
  return RBL_OK;
}
float* slotp32(rbl_ctx* ctx, int j) {
  const int s = j < ctx->resident ? j : ctx->resident + (j & 1);
  return ctx->d_basis32 + (int64_t)s * ctx->slot;
}
const float* block_dev32(rbl_ctx* ctx, int j, int nblocks, int* st) {
  *st = 0;
  if (j < ctx->resident || j >= nblocks - 2) return slotp32(ctx, j);
  const hipError_t e = hipMemcpyAsync(ctx->d_stage32, ctx->h_spill[j - ctx->resident],
                                      ctx->slot * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) *st = RBL_ERR_HIP;
  return ctx->d_stage32;
}

CsrDev csr(rbl_ctx* ctx) {
  CsrDev A;
  A.nrows = ctx->nloc;
  A.nnz = ctx->nnz;
  A.rowptr = ctx->d_rowptr;
  A.col = ctx->d_col;
  A.val = ctx->d_val;
  A.tile_cmin = ctx->d_tcmin;
  A.tile_cmax = ctx->d_tcmax;
  A.tile_info = ctx->d_tinfo;
  // (the indexed halo's buffer holds ghost slots, not a row range: the panels need the range)
  A.panel_blk = ctx->ghost ? nullptr : ctx->d_panel_blk;
  A.panel_nblk = ctx->ghost ? 0 : ctx->panel_nblk;
  A.panel_auto = ctx->panel_auto;
  A.panel_cnt = ctx->d_panel_cnt;
  A.panel_st = ctx->d_panel_st;
  A.panel_col = ctx->d_panel_col;
  A.panel_val = ctx->d_panel_val;
  A.panel_rpg = ctx->panel_rpg;
  A.panel_ch = ctx->panel_ch;
  A.ntiles = ctx->ntiles;
  A.tiles_per_wg = ctx->tiles_per_wg;
  A.window_ok16 = ctx->window_ok16;
  A.window_ok32 = ctx->window_ok32;
  A.band_ok16 = ctx->band_ok16;
  A.band_ok32 = ctx->band_ok32;
  A.band_gram = ctx->band_gram;
  A.band_pair = ctx->band_pair;
  A.row0 = ctx->r0;
  A.band_pos = ctx->d_bpos;
  A.bt = ctx->d_bt;
  A.bth = ctx->d_bth;
  A.bte = ctx->d_bte;
  A.bt_ng = ctx->bt_ng;
  A.btp_hdr = ctx->d_btp_hdr;
  A.btp_val = ctx->d_btp_val;
  A.bt_tiles_per_wg = ctx->tiles_per_wg;
  A.q_lo = ctx->nranks > 1 ? ctx->ext_lo : ctx->r0;
  A.q_hi = ctx->nranks > 1 ? ctx->ext_hi : ctx->r0 + ctx->nloc;
  A.zrow = ctx->d_zrow;
  A.seg_ntasks = ctx->seg_ntasks;
  A.seg_trow = ctx->d_seg_trow;
  A.seg_tinfo = ctx->d_seg_tinfo;
  A.seg_slot_k0 = ctx->d_seg_slot_k0;
  A.seg_nlong = ctx->seg_nlong;
  A.seg_lrow = ctx->d_seg_lrow;
  A.seg_lslot = ctx->d_seg_lslot;
  A.seg_scratch = ctx->d_seg_scratch;
  A.seg_ntiers = ctx->seg_ntiers;
  A.seg_split = ctx->seg_split;
  for (int t = 0; t < ctx->seg_ntiers; ++t) {
    const auto& T = ctx->seg_tier[t];
    auto& D = A.seg_tier[t];
    D.rowptr = T.rowptr;
    D.col = T.col;
    D.val = T.val;
    D.ntasks = T.ntasks;
    D.nlong = T.nlong;
    D.trow = T.trow;
    D.tinfo = T.tinfo;
    D.slot_k0 = T.slot_k0;
    D.lrow = T.lrow;
    D.lslot = T.lslot;
    D.scratch = T.scratch;
  }
  return A;
}

// Task table of the segmented gather (spmm.hip variant 5): short rows packed into tasks of
// <= kSegPack nonzeros and <= 64 rows, rows over kSegLen nonzeros cut into segments.  The
// rectangular gather pair (spmm_rect.hip) builds its two tables here with its own limits and
// scratch_w = 64 doubles per segment slot.
int build_seg(rbl_ctx* ctx, const std::vector<int64_t>& rp, SegTierBuf& out,
              int64_t seg_len = kSegLen, int64_t pack = kSegPack, int scratch_w = 32) {
  const int64_t m = (int64_t)rp.size() - 1;
  if (m <= 0) return RBL_OK;
  std::vector<int64_t> trow, slot_k0, lrow, lslot;
  std::vector<int32_t> tinfo;
  int64_t cur_r0 = 0, cur_nnz = 0;
  int cur_rows = 0;
  auto flush = [&]() {
    if (cur_rows) {
      trow.push_back(cur_r0);
      tinfo.push_back(cur_rows);
    }
    cur_rows = 0;
    cur_nnz = 0;
  };
  for (int64_t r = 0; r < m; ++r) {
    const int64_t d = rp[r + 1] - rp[r];
    if (d > seg_len) {
      flush();
      lrow.push_back(r);
      lslot.push_back((int64_t)slot_k0.size());
      for (int64_t k = rp[r]; k < rp[r + 1]; k += seg_len) {
        trow.push_back(r);
        tinfo.push_back(-(int32_t)(slot_k0.size() + 1));
        slot_k0.push_back(k);
      }
      continue;
    }
    if (cur_rows && (cur_nnz + d > pack || cur_rows == 64)) flush();
    if (!cur_rows) cur_r0 = r;
    ++cur_rows;
    cur_nnz += d;
  }
  flush();
  lslot.push_back((int64_t)slot_k0.size());
  slot_k0.push_back(INT64_MAX);
  out.ntasks = (int64_t)trow.size();
  out.nlong = (int64_t)lrow.size();
  HIPC(out.trow.alloc(trow.size()));
  HIPC(out.tinfo.alloc(tinfo.size()));
  HIPC(out.slot_k0.alloc(slot_k0.size()));
  HIPC(out.lslot.alloc(lslot.size()));
  HIPC(out.lrow.alloc(std::max<size_t>(lrow.size(), 1)));
  HIPC(out.scratch.alloc(std::max<size_t>(slot_k0.size() - 1, 1) * scratch_w));
  HIPC(hipMemcpy(out.trow, trow.data(), trow.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(out.tinfo, tinfo.data(), tinfo.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(out.slot_k0, slot_k0.data(), slot_k0.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(out.lslot, lslot.data(), lslot.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  if (!lrow.empty())
    HIPC(hipMemcpy(out.lrow, lrow.data(), lrow.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  return RBL_OK;
}

// the column-panel format (spmm_panel.hip) and its choice
void free_panels(rbl_ctx* ctx) {
  static_cast<PanelBufs&>(*ctx) = PanelBufs{};
  ctx->panel_nblk = 0;
  ctx->panel_auto = false;
  ctx->panel_span = 0;
}

void free_tiers(rbl_ctx* ctx) {
  static_cast<TierBufs&>(*ctx) = TierBufs{};
  ctx->seg_ntiers = 0;
  ctx->seg_split = false;
  ctx->ghost = false;
  ctx->n_ghost = ctx->n_send = 0;
  ctx->push = false;
  ctx->push_rows = 0;
  ctx->n_ps_rows = 0;
}

int prepare_segments(rbl_ctx* ctx, const std::vector<int64_t>& rp) {
  if (ctx->nloc <= 0 || ctx->nnz <= 0) return RBL_OK;
  SegTierBuf T;
  const int st = build_seg(ctx, rp, T);
  ctx->seg_ntasks = T.ntasks;
  ctx->seg_nlong = T.nlong;
  ctx->d_seg_trow = std::move(T.trow);
  ctx->d_seg_tinfo = std::move(T.tinfo);
  ctx->d_seg_slot_k0 = std::move(T.slot_k0);
  ctx->d_seg_lrow = std::move(T.lrow);
  ctx->d_seg_lslot = std::move(T.lslot);
  ctx->d_seg_scratch = std::move(T.scratch);
  return st;
}

int build_tiers(rbl_ctx* ctx, const std::vector<uint8_t>& tier_of, int nt,
                const TierRule* rule = nullptr);

// nonzeros of tier t (its row pointer's last entry)
int64_t tier_nnz(rbl_ctx* ctx, int t) {
  int64_t v = 0;
  if (ctx->seg_tier[t].rowptr && ctx->nloc > 0)
    (void)hipMemcpy(&v, ctx->seg_tier[t].rowptr + ctx->nloc, sizeof(int64_t), hipMemcpyDeviceToHost);
  return v;
}

// Indexed halo: the columns this rank references outside its rows become ghost slots (sorted by
// global id, so grouped by owner); the ranks exchange how many rows, then which rows, each asks
// of each; d_map (device, n int32) maps a ghost column to its slot.
int build_ghosts(rbl_ctx* ctx, DevBuf<int32_t>& d_map, const int32_t* cols, int64_t ncols) {
  const int P = ctx->nranks, me = ctx->rank;
  const int64_t n = ctx->n;
  DevBuf<uint8_t> d_mark;
  HIPC(d_mark.alloc(std::max<int64_t>(n, 1)));
  HIPC(hipMemsetAsync(d_mark, 0, n, ctx->stream));
  mark_cols(cols, ncols, ctx->r0, ctx->r1, d_mark, ctx->stream);
  HIPC(hipGetLastError());
  std::vector<uint8_t> mark(n);
  HIPC(hipMemcpyAsync(mark.data(), d_mark, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  d_mark.reset();  // n bytes, before the host map and d_map of n int32 each
  std::vector<int32_t> map(n, 0);
  std::vector<int64_t> req;  // global ids of the ghost rows, ascending
  ctx->ghost_cnt.assign(P, 0);
  ctx->ghost_off.assign(P, 0);
  for (int q = 0; q < P; ++q) {
    ctx->ghost_off[q] = (int64_t)req.size();
    if (q == me) continue;
    for (int64_t c = ctx->bounds[q]; c < ctx->bounds[q + 1]; ++c)
      if (mark[c]) {
        map[c] = (int32_t)req.size();
        req.push_back(c);
      }
    ctx->ghost_cnt[q] = (int64_t)req.size() - ctx->ghost_off[q];
  }
  ctx->n_ghost = (int64_t)req.size();
  // what each peer asks of me: row `me` of the all-gathered count table, column by column
  std::vector<int64_t> all((size_t)P * P);
  COMMC(ctx->comm->allgather_host(ctx->ghost_cnt.data(), all.data(), P, ctx->stream, &ctx->err));
  ctx->send_cnt.assign(P, 0);
  ctx->send_off.assign(P, 0);
  int64_t ns = 0;
  for (int q = 0; q < P; ++q) {
    ctx->send_off[q] = ns;
    ctx->send_cnt[q] = q == me ? 0 : all[(size_t)q * P + me];
    ns += ctx->send_cnt[q];
  }
  ctx->n_send = ns;
  // the request lists themselves, int64 ids carried as 8-byte words by the halo transport
  DevBuf<int64_t> d_req, d_got;
  HIPC(d_req.alloc(std::max<int64_t>(ctx->n_ghost, 1)));
  HIPC(d_got.alloc(std::max<int64_t>(ns, 1)));
  if (ctx->n_ghost)
    HIPC(hipMemcpy(d_req, req.data(), ctx->n_ghost * sizeof(int64_t), hipMemcpyHostToDevice));
  std::vector<Comm::Xfer> x(P);
  for (int q = 0; q < P; ++q) {
    if (q == me) continue;
    x[q].send = reinterpret_cast<const double*>(d_req + ctx->ghost_off[q]);
    x[q].nsend = (size_t)ctx->ghost_cnt[q];
    x[q].recv = reinterpret_cast<double*>(d_got + ctx->send_off[q]);
    x[q].nrecv = (size_t)ctx->send_cnt[q];
  }
  COMMC(ctx->comm->exchange(x, ctx->stream, &ctx->err));
  std::vector<int64_t> got(std::max<int64_t>(ns, 1));
  HIPC(hipMemcpyAsync(got.data(), d_got, ns * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  std::vector<int32_t> idx(std::max<int64_t>(ns, 1), 0);
  for (int64_t i = 0; i < ns; ++i) {
    const int64_t g = got[i] - ctx->r0;
    if (g < 0 || g >= ctx->nloc) return fail(ctx, RBL_ERR_INVALID, "indexed halo: a peer asked for a row I do not own");
    idx[i] = (int32_t)g;
  }
  HIPC(ctx->d_send_idx.alloc(std::max<int64_t>(ns, 1)));
  if (ns) HIPC(hipMemcpy(ctx->d_send_idx, idx.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPC(d_map.alloc(std::max<int64_t>(n, 1)));
  HIPC(hipMemcpy(d_map, map.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  return RBL_OK;
}

// Push/pull split of the indexed halo (several ranks, unbanded A).  Every off-rank product
// A[r,c] Q[c] is done by the rank of the endpoint that ranks higher by (row degree, smaller id):
// when c ranks higher the rank of r pulls Q[c] (tier 1, as in the pull-all halo), otherwise the
// rank of c — which holds A[c,r] = A[r,c] in its own rows — forms it from its own Q rows and
// pushes the partial row r (tier 2 is dropped: its products arrive pushed).  Hub rows (the
// high-degree rows of a power-law graph, referenced from every rank) then stay home and only
// their partials move, one row per (hub, rank) pair in each direction.  The push tier is tier
// 1 transposed (rows: the ghost slots, columns: own rows), so ghosts pulled = partials pushed.
// Returns 1 when set up, 0 when the pull-all halo is to be used — off (RBL_OPT_HALO_PUSH 0),
// predicted to move more rows (automatic: used when 2 x ghosts(tier 1) < 0.85 x ghosts(all),
// summed over ranks), or A not structurally symmetric by the per-pair entry counts — the
// same answer on every rank; < 0 on error.  Collective.
int prepare_push(rbl_ctx* ctx, const std::vector<int64_t>& rp) {
  const int P = ctx->nranks;
  const int64_t n = ctx->n, m = ctx->nloc;
  // global row degrees: every rank's slice (padded to the longest) all-gathered
  int64_t w = 1;
  for (int q = 0; q < P; ++q) w = std::max(w, ctx->bounds[q + 1] - ctx->bounds[q]);
  std::vector<int64_t> mine(w, 0), all((size_t)P * w);
  for (int64_t r = 0; r < m && r + 1 < (int64_t)rp.size(); ++r) mine[r] = rp[r + 1] - rp[r];
  COMMC(ctx->comm->allgather_host(mine.data(), all.data(), w, ctx->stream, &ctx->err));
  std::vector<int32_t> deg(std::max<int64_t>(n, 1), 0);
  for (int q = 0; q < P; ++q)
    for (int64_t i = 0; i < ctx->bounds[q + 1] - ctx->bounds[q]; ++i)
      deg[ctx->bounds[q] + i] = (int32_t)std::min<int64_t>(all[(size_t)q * w + i], INT32_MAX);
  std::vector<int64_t>().swap(all);
  DevBuf<int32_t> d_deg;
  HIPC(d_deg.alloc(deg.size()));
  HIPC(hipMemcpy(d_deg, deg.data(), deg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  TierRule R;
  R.deg = d_deg;
  R.row0 = ctx->r0;
  R.r0 = ctx->r0;
  R.r1 = ctx->r1;
  CHK(build_tiers(ctx, {}, 3, &R));
  // per peer: my tier-1 / tier-2 entries by the owner of their column, and the distinct
  // columns of tier 1 (the ghosts with the split) and of tiers 1 + 2 (without)
  const int64_t nz1 = m > 0 ? tier_nnz(ctx, 1) : 0, nz2 = m > 0 ? tier_nnz(ctx, 2) : 0;
  std::vector<int32_t> c1(std::max<int64_t>(nz1, 1)), c2(std::max<int64_t>(nz2, 1));
  // [tier-1 entries by owner | tier-2 by owner | d1 | d12 | tier-1 hash by owner | tier-2 hash |
  //  this rank's status]: a rank whose local part fails (a D2H copy) still takes part in the
  // all-gather with its error code, and every rank then fails together instead of leaving its
  // peers waiting in the collective
  std::vector<int64_t> vote(4 * P + 3, 0);
  auto owner = [&](int64_t c) {
    return (int)(std::upper_bound(ctx->bounds.begin(), ctx->bounds.end(), c) - ctx->bounds.begin()) - 1;
  };
  auto local_counts = [&]() -> int {
    if (nz1) HIPC(hipMemcpy(c1.data(), ctx->seg_tier[1].col, nz1 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (nz2) HIPC(hipMemcpy(c2.data(), ctx->seg_tier[2].col, nz2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<uint8_t> mark(std::max<int64_t>(n, 1), 0);
    for (int64_t k = 0; k < nz1; ++k) {
      ++vote[owner(c1[k])];
      if (!mark[c1[k]]) { mark[c1[k]] = 1; ++vote[2 * P]; }
    }
    for (int64_t k = 0; k < nz2; ++k) {
      ++vote[P + owner(c2[k])];
      if (!mark[c2[k]]) { mark[c2[k]] = 2; ++vote[2 * P + 1]; }
    }
    vote[2 * P + 1] += vote[2 * P];
    std::vector<uint8_t>().swap(mark);
    // the entries themselves, not only their counts: the split forms A[r,c] Q[c] on c's rank from
    // A[c,r], so p's tier-2 entries towards q must be q's tier-1 entries towards p transposed,
    // values included.  Per peer an order-free hash (wrapping sum of mixed (row, col, value
    // bits), tier 2 keyed transposed) is compared: a pattern or a value that is not symmetric
    // keeps the pull-all halo (or fails under RBL_OPT_HALO_PUSH 1) instead of a wrong SpMM.
    auto tier_hash = [&](int t, int64_t nz, const std::vector<int32_t>& cols, int64_t* out) -> int {
      if (nz == 0) return RBL_OK;
      std::vector<int64_t> trp(m + 1);
      std::vector<double> tv(nz);
      HIPC(hipMemcpy(trp.data(), ctx->seg_tier[t].rowptr, (m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
      HIPC(hipMemcpy(tv.data(), ctx->seg_tier[t].val, nz * sizeof(double), hipMemcpyDeviceToHost));
      for (int64_t r = 0; r < m; ++r)
        for (int64_t k = trp[r]; k < trp[r + 1]; ++k) {
          const uint64_t row = (uint64_t)(ctx->r0 + r), col = (uint64_t)cols[k];
          uint64_t vb;
          memcpy(&vb, &tv[k], sizeof(vb));
          const uint64_t a = t == 1 ? row : col, b2 = t == 1 ? col : row;  // tier 2: transposed
          const uint64_t h = mix64(mix64(a * 0x9E3779B97F4A7C15ull ^ b2) ^ vb);
          out[owner(cols[k])] = (int64_t)((uint64_t)out[owner(cols[k])] + h);
        }
      return RBL_OK;
    };
    CHK(tier_hash(1, nz1, c1, vote.data() + 2 * P + 2));
    CHK(tier_hash(2, nz2, c2, vote.data() + 3 * P + 2));
    return RBL_OK;
  };
  const int lrc = local_counts();
  std::vector<int32_t>().swap(c2);
  const int V = 4 * P + 3;
  vote[4 * P + 2] = lrc;
  std::vector<int64_t> votes((size_t)P * V);
  COMMC(ctx->comm->allgather_host(vote.data(), votes.data(), V, ctx->stream, &ctx->err));
  if (lrc < 0) return lrc;  // (ctx->err already says what failed here)
  for (int p = 0; p < P; ++p)
    if (votes[(size_t)p * V + 4 * P + 2] < 0)
      return fail(ctx, (int)votes[(size_t)p * V + 4 * P + 2],
                  "push/pull halo setup failed on rank " + std::to_string(p));
  bool sym = true;
  int64_t d1 = 0, d12 = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t* vp = votes.data() + (size_t)p * V;
    d1 += vp[2 * P];
    d12 += vp[2 * P + 1];
    for (int q = 0; q < P; ++q) {  // p's tier-2 entries towards q are q's tier-1 entries towards p
      const int64_t* vq = votes.data() + (size_t)q * V;
      if (vp[P + q] != vq[p] || vp[3 * P + 2 + q] != vq[2 * P + 2 + p]) sym = false;
    }
  }
  ctx->push_pred_rows = 2 * d1;
  ctx->pull_pred_rows = d12;
  if (!sym) {
    if (ctx->halo_push_opt == 1)
      return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_HALO_PUSH: A is not symmetric (pattern or values)");
    return 0;
  }
  if (ctx->halo_push_opt == 2 && !(2.0 * (double)d1 < 0.85 * (double)d12)) return 0;
  // split: tier 2 dropped, the ghosts are tier 1's columns
  ctx->seg_tier[2] = SegTierBuf();
  ctx->seg_ntiers = 2;
  DevBuf<int32_t> d_map;
  CHK(build_ghosts(ctx, d_map, ctx->seg_tier[1].col, nz1));
  if (nz1) remap_cols(ctx->seg_tier[1].col, nz1, d_map, ctx->stream);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->seg_split = true;
  ctx->ghost = true;
  // the push tier: tier 1 transposed, rows = ghost slots (in row order within a slot)
  const int64_t G = ctx->n_ghost;
  std::vector<int64_t> rp1(m + 1, 0);
  std::vector<double> v1(std::max<int64_t>(nz1, 1));
  if (m > 0) HIPC(hipMemcpy(rp1.data(), ctx->seg_tier[1].rowptr, (m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (nz1) {
    HIPC(hipMemcpy(c1.data(), ctx->seg_tier[1].col, nz1 * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(v1.data(), ctx->seg_tier[1].val, nz1 * sizeof(double), hipMemcpyDeviceToHost));
  }
  std::vector<int64_t> prp(G + 1, 0);
  for (int64_t k = 0; k < nz1; ++k) ++prp[c1[k] + 1];
  for (int64_t g = 0; g < G; ++g) prp[g + 1] += prp[g];
  std::vector<int64_t> pos(prp.begin(), prp.end() - 1);
  std::vector<int32_t> pc(std::max<int64_t>(nz1, 1));
  std::vector<double> pv(std::max<int64_t>(nz1, 1));
  for (int64_t r = 0; r < m; ++r)
    for (int64_t k = rp1[r]; k < rp1[r + 1]; ++k) {
      const int64_t at = pos[c1[k]]++;
      pc[at] = (int32_t)(ctx->r0 + r);
      pv[at] = v1[k];
    }
  auto& T = ctx->push_tier;
  HIPC(T.rowptr.alloc(G + 1));
  HIPC(T.col.alloc(nz1 + kCsrPad));
  HIPC(T.val.alloc(nz1 + kCsrPad));
  HIPC(hipMemset(T.col, 0, (nz1 + kCsrPad) * sizeof(int32_t)));
  HIPC(hipMemset(T.val, 0, (nz1 + kCsrPad) * sizeof(double)));
  HIPC(hipMemcpy(T.rowptr, prp.data(), (G + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (nz1) {
    HIPC(hipMemcpy(T.col, pc.data(), nz1 * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(T.val, pv.data(), nz1 * sizeof(double), hipMemcpyHostToDevice));
  }
  CHK(build_seg(ctx, prp, T));
  ctx->push_rows = G;
  // where the received partials go: the own rows asked for, each with its slots in peer order
  const int64_t ns = ctx->n_send;
  std::vector<int32_t> sidx(std::max<int64_t>(ns, 1));
  if (ns) HIPC(hipMemcpy(sidx.data(), ctx->d_send_idx, ns * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int64_t> cnt(std::max<int64_t>(m, 1) + 1, 0);
  for (int64_t k = 0; k < ns; ++k) ++cnt[sidx[k] + 1];
  for (int64_t r = 0; r < m; ++r) cnt[r + 1] += cnt[r];
  std::vector<int64_t> slot(std::max<int64_t>(ns, 1)), rows, ptr(1, 0);
  {
    std::vector<int64_t> at(cnt.begin(), cnt.end() - 1);
    for (int64_t k = 0; k < ns; ++k) slot[at[sidx[k]]++] = k;
  }
  for (int64_t r = 0; r < m; ++r)
    if (cnt[r + 1] > cnt[r]) {
      rows.push_back(r);
      ptr.push_back(cnt[r + 1]);
    }
  ctx->n_ps_rows = (int64_t)rows.size();
  HIPC(ctx->d_ps_rows.alloc(std::max<size_t>(rows.size(), 1)));
  HIPC(ctx->d_ps_ptr.alloc(ptr.size()));
  HIPC(ctx->d_ps_slot.alloc(slot.size()));
  if (!rows.empty())
    HIPC(hipMemcpy(ctx->d_ps_rows, rows.data(), rows.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->d_ps_ptr, ptr.data(), ptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->d_ps_slot, slot.data(), slot.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  ctx->push = true;
  return 1;
}

// Column tiers of the segmented gather (RBL_SEG_TIERS="h[,w]": the h highest-degree columns,
// then the next w, then the rest; one rank, A symmetric so a column's degree is its row's).
// The SpMM sweeps the tiers in order; each sweep's gathers hit a Q-row set sized for one cache
// level.  Results differ from the one-sweep SpMM only in the order of each row's sum.
// Several ranks (unbanded A, the segmented gather): two tiers instead, the own columns
// [r0, r1) and the halo columns, so the own part of the SpMM runs while the halo exchange is in
// flight (step_impl); the sum order per row is the same with or without the overlap.
// the column panels on several ranks need the range halo: taken where every block's window
// is a small part of the matrix (a band), not where the windows span it (a small R-MAT's blocks
// may pass panel_auto, and its indexed halo moves fewer rows)
bool panel_banded(const rbl_ctx* ctx) { return ctx->panel_auto && 4 * ctx->panel_span <= ctx->n; }

int prepare_tiers(rbl_ctx* ctx, const std::vector<int64_t>& rp) {
  free_tiers(ctx);
  ctx->push_pred_rows = ctx->pull_pred_rows = 0;
  if (ctx->nranks > 1) {
    // every rank must take the same branch (the setup below runs collectives), so the vote
    // comes before any per-rank condition: a rank with no rows or no nonzeros still takes
    // part in build_ghosts (with no requests), and a rank that released its CSR for band tiles
    // (RBL_OPT_KEEP_CSR = 0) votes banded, which stops every rank here
    const int64_t banded = (ctx->bt_ng || ctx->band_ok16 || ctx->band_ok32 || ctx->window_ok16 ||
                            ctx->window_ok32 || panel_banded(ctx) || ctx->dense || ctx->csr_dropped)
                               ? 1 : 0;
    std::vector<int64_t> all(ctx->nranks);
    COMMC(ctx->comm->allgather_host(&banded, all.data(), 1, ctx->stream, &ctx->err));
    for (int64_t v : all)
      if (v) return RBL_OK;  // a banded kernel runs: its halo is a range of rows
    std::vector<uint8_t> tier_of(ctx->n, 1);
    for (int64_t c = ctx->r0; c < ctx->r1; ++c) tier_of[c] = 0;
    if (ctx->halo_push_opt != 0) {  // the push/pull split, if it moves fewer rows (collective)
      const int ps = prepare_push(ctx, rp);
      if (ps < 0) return ps;
      if (ps == 1) return RBL_OK;
      free_tiers(ctx);
    }
    DevBuf<int32_t> d_map;
    CHK(build_ghosts(ctx, d_map, ctx->d_col, ctx->nnz));
    const int st = build_tiers(ctx, tier_of, 2);
    if (st == RBL_OK) {
      remap_cols(ctx->seg_tier[1].col, ctx->seg_tier[1].ntasks > 0 ? tier_nnz(ctx, 1) : 0, d_map,
                 ctx->stream);
      HIPC(hipGetLastError());
      HIPC(hipStreamSynchronize(ctx->stream));
    }
    CHK(st);
    ctx->seg_split = true;
    ctx->ghost = true;
    // the rows this halo moves per SpMM, summed over ranks (rbl_comm_stats' halo plan)
    std::vector<int64_t> ng(ctx->nranks);
    COMMC(ctx->comm->allgather_host(&ctx->n_ghost, ng.data(), 1, ctx->stream, &ctx->err));
    ctx->pull_pred_rows = 0;
    for (int64_t v : ng) ctx->pull_pred_rows += v;
    return RBL_OK;
  }
  if (ctx->seg_ntasks == 0 || ctx->nnz == 0 || ctx->csr_dropped) return RBL_OK;
#ifndef RBL_VARIANTS
  return RBL_OK;
#else
  // (variants build only: the degree-ranked column tiers of one rank, measured no faster,
  // DESIGN.md §3 round 3)
  const char* e = std::getenv("RBL_SEG_TIERS");
  if (!e || ctx->nloc != ctx->n) return RBL_OK;
  std::vector<int64_t> sz;
  for (const char* p = e; *p;) {
    char* end = nullptr;
    const long long v = std::strtoll(p, &end, 10);
    if (end == p) break;
    if (v > 0) sz.push_back(v);
    p = *end == ',' ? end + 1 : end;
    if (sz.size() == kMaxSegTiers - 1) break;
  }
  if (sz.empty()) return RBL_OK;
  const int nt = (int)sz.size() + 1;
  const int64_t n = ctx->n, m = ctx->nloc;
  std::vector<int64_t> order(n);
  for (int64_t c = 0; c < n; ++c) order[c] = c;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b2) {
    return rp[a + 1] - rp[a] > rp[b2 + 1] - rp[b2];
  });
  std::vector<uint8_t> tier_of(n, (uint8_t)(nt - 1));
  int64_t rank = 0;
  for (int t = 0; t < nt - 1; ++t)
    for (int64_t k = 0; k < sz[t] && rank < n; ++k) tier_of[order[rank++]] = (uint8_t)t;
  (void)m;
  return build_tiers(ctx, tier_of, nt);
#endif
}

// The tier CSRs and task tables for a column -> tier map (tier_of: n entries, < nt), or for
// the per-nonzero rule of the push/pull halo split (rule, nt = 3).
int build_tiers(rbl_ctx* ctx, const std::vector<uint8_t>& tier_of, int nt, const TierRule* rule) {
  const int64_t n = ctx->n, m = ctx->nloc;
  DevBuf<uint8_t> d_tier;
  DevBuf<int32_t> d_cnt;
  HIPC(d_tier.alloc(rule ? 1 : n));
  HIPC(d_cnt.alloc(std::max<size_t>((size_t)nt * m, 1)));
  if (rule)
    seg_tier_count_rule(m, ctx->d_rowptr, ctx->d_col, *rule, d_cnt, ctx->stream);
  else {
    HIPC(hipMemcpy(d_tier, tier_of.data(), n, hipMemcpyHostToDevice));
    seg_tier_count(m, ctx->d_rowptr, ctx->d_col, d_tier, nt, d_cnt, ctx->stream);
  }
  HIPC(hipGetLastError());
  std::vector<int32_t> cnt((size_t)nt * m);
  HIPC(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  std::vector<std::vector<int64_t>> trp(nt, std::vector<int64_t>(m + 1, 0));
  int64_t* rpp[kMaxSegTiers] = {nullptr, nullptr, nullptr};
  int32_t* colp[kMaxSegTiers] = {nullptr, nullptr, nullptr};
  double* valp[kMaxSegTiers] = {nullptr, nullptr, nullptr};
  for (int t = 0; t < nt; ++t) {
    for (int64_t r = 0; r < m; ++r) trp[t][r + 1] = trp[t][r] + cnt[(size_t)t * m + r];
    auto& T = ctx->seg_tier[t];
    const int64_t nz = trp[t][m];
    HIPC(T.rowptr.alloc(m + 1));
    HIPC(T.col.alloc(nz + kCsrPad));
    HIPC(T.val.alloc(nz + kCsrPad));
    HIPC(hipMemset(T.col + nz, 0, kCsrPad * sizeof(int32_t)));
    HIPC(hipMemset(T.val + nz, 0, kCsrPad * sizeof(double)));
    HIPC(hipMemcpy(T.rowptr, trp[t].data(), (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    rpp[t] = T.rowptr;
    colp[t] = T.col;
    valp[t] = T.val;
  }
  ctx->seg_ntiers = nt;  // (free_tiers releases partial state on a later failure)
  if (rule)
    seg_tier_fill_rule(m, ctx->d_rowptr, ctx->d_col, ctx->d_val, *rule, rpp, colp, valp, ctx->stream);
  else
    seg_tier_fill(m, ctx->d_rowptr, ctx->d_col, ctx->d_val, d_tier, nt, rpp, colp, valp, ctx->stream);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int t = 0; t < nt; ++t) CHK(build_seg(ctx, trp[t], ctx->seg_tier[t]));
  return RBL_OK;
}

// Per-16-row-tile column footprint for the LDS-window SpMM and the checks that every tile
// fits its ring (spmm_window.hip): columns sorted per row, footprints non-decreasing, a
// tile's nonzeros <= 2048, ring rows: 256 (b=32) / 512 (b=16), new rows per tile <= 32 / 64.
int prepare_window_formats(rbl_ctx* ctx, const std::vector<int64_t>& rp);
// the column-panel SpMM's limit: panels per row block (256-row panels: windows <= 16 K rows)
constexpr int64_t kPanelMax = 64;
// Every SpMM format of a freshly set CSR: the segmented-gather table, the window / band /
// band-tile formats, then (unbanded only) the column tiers.
int prepare_window(rbl_ctx* ctx, const std::vector<int64_t>& rp) {
  CHK(prepare_window_formats(ctx, rp));
  CHK(prepare_tiers(ctx, rp));  // (collective on several ranks: every rank calls it)
  return RBL_OK;
}

int prepare_window_formats(rbl_ctx* ctx, const std::vector<int64_t>& rp) {
  CHK(prepare_segments(ctx, rp));
  ctx->window_ok16 = ctx->window_ok32 = false;
  ctx->band_ok16 = ctx->band_ok32 = false;
  ctx->band_gram = false;
  ctx->band_pair = false;
  ctx->ntiles = (ctx->nloc + kWindowTileRows - 1) / kWindowTileRows;
  if (ctx->ntiles == 0 || ctx->nnz == 0) return RBL_OK;
  const int64_t nt = ctx->ntiles;
  HIPC(ctx->d_tcmin.alloc(nt));
  HIPC(ctx->d_tcmax.alloc(nt));
  CsrDev A;
  A.nrows = ctx->nloc;
  A.rowptr = ctx->d_rowptr;
  A.col = ctx->d_col;
  tile_col_range(A, kWindowTileRows, ctx->d_tcmin, ctx->d_tcmax, ctx->stream);
  std::vector<int64_t> cmin(nt), cmax(nt);
  HIPC(hipMemcpyAsync(cmin.data(), ctx->d_tcmin, nt * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(cmax.data(), ctx->d_tcmax, nt * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  // band-tile kernel (spmm_bt.hip): every nonempty tile's columns within
  // [r0 + 16t - H, r0 + 16t + 16 + H) for H = 32 or 64
  int64_t hneed = 0;
  for (int64_t t = 0; t < nt; ++t) {
    if (cmax[t] < 0) continue;
    const int64_t ra = ctx->r0 + t * kWindowTileRows;
    hneed = std::max(hneed, std::max(ra - cmin[t], cmax[t] - (ra + kWindowTileRows - 1)));
  }
  // forward-fill empty tiles (cmax < 0), then backward-fill leading empties
  int64_t first = -1;
  for (int64_t t = 0; t < nt; ++t) {
    if (cmax[t] < 0) {
      if (t > 0) { cmin[t] = cmin[t - 1]; cmax[t] = cmax[t - 1]; }
    } else if (first < 0) {
      first = t;
    }
  }
  if (first < 0) return RBL_OK;
  for (int64_t t = 0; t < first; ++t) { cmin[t] = cmin[first]; cmax[t] = cmax[first]; }
  bool ok = true;
  int64_t max_span = 0, max_new = 0;
  for (int64_t t = 0; t < nt && ok; ++t) {
    const int64_t ra = t * kWindowTileRows;
    const int64_t rb = std::min(ra + kWindowTileRows, ctx->nloc);
    if (rp[rb] - rp[ra] > 2048) ok = false;
    max_span = std::max(max_span, cmax[t] + 1 - cmin[t]);
    if (t > 0) {
      if (cmin[t] < cmin[t - 1] || cmax[t] < cmax[t - 1]) ok = false;
      max_span = std::max(max_span, cmax[t] + 1 - cmin[t - 1]);
      max_new = std::max(max_new, cmax[t] - std::max(cmax[t - 1], cmin[t] - 1));
    }
  }
  ctx->window_ok32 = ok && max_span <= 256 && max_new <= 32;
  ctx->window_ok16 = ok && max_span <= 512 && max_new <= 64;
  // band (MFMA) kernel (spmm_band.hip): tile band [c16, cmax] (c16 = cmin & ~15) at most
  // kBandMaxK columns, rows <= 192 nonzeros, and the dense tiles at least 25 % filled (else
  // the zero padding costs more than it saves)
  {
    int64_t max_row = 0, dense = 0, max_k = 0;
    for (int64_t i = 0; i < ctx->nloc; ++i) max_row = std::max(max_row, rp[i + 1] - rp[i]);
    for (int64_t t = 0; t < nt; ++t) {
      const int64_t k = cmax[t] + 1 - (cmin[t] & ~int64_t(15));
      max_k = std::max(max_k, k);
      dense += kWindowTileRows * ((k + 15) / 16 * 16);
    }
    // producers write tile t+2's new ring rows while tile t is multiplied: the ring must hold
    // [cmin(t), cmax(t+2)]
    int64_t max_span2 = 0;
    for (int64_t t = 0; t < nt; ++t)
      max_span2 = std::max(max_span2, cmax[std::min(t + 2, nt - 1)] + 1 - cmin[t]);
    const bool bok = ok && max_span2 <= kBandRing && max_k <= kBandMaxK && max_row <= 192 &&
                     4 * ctx->nnz >= dense;
    ctx->band_ok32 = bok && max_new <= 32;
    ctx->band_ok16 = bok && max_new <= 64;
    // A_i = Q^T U inside the band kernel reads Q's tile rows from the ring: each tile's own
    // (global) rows must lie in its band, and stay resident until the tile's U is final (one
    // phase late at b=16): rows [r(t), r(t)+16) vs the ring's [cmin(t), cmax(t+3)]
    bool gok = bok;
    for (int64_t t = 0; t < nt && gok; ++t) {
      const int64_t ra = ctx->r0 + t * kWindowTileRows;
      const int64_t rb = ctx->r0 + std::min((t + 1) * kWindowTileRows, ctx->nloc) - 1;
      if (ra < cmin[t] || rb > cmax[t]) gok = false;
      if (cmax[std::min(t + 3, nt - 1)] + 1 - ra > kBandRing) gok = false;
    }
    ctx->band_gram = gok;
    // rows (2p, 2p+1) of every 16-row tile: nonzeros + up to 3 of alignment shift <= 256
    int64_t max_pair = 0;
    for (int64_t r = 0; r < ctx->nloc; r += 2)
      max_pair = std::max(max_pair, rp[std::min(r + 2, ctx->nloc)] - rp[r]);
    ctx->band_pair = bok && max_pair + 3 <= 256;
  }
  HIPC(hipMemcpy(ctx->d_tcmin, cmin.data(), nt * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->d_tcmax, cmax.data(), nt * sizeof(int64_t), hipMemcpyHostToDevice));
  std::vector<int64_t> info(8 * nt, 0);
  for (int64_t t = 0; t < nt; ++t) {
    const int64_t ra = t * kWindowTileRows;
    const int64_t rb = std::min(ra + kWindowTileRows, ctx->nloc);
    int64_t lo = cmin[t];
    if (t > 0) lo = std::max(lo, cmax[t - 1] + 1);
    const int64_t hi = std::max(lo, cmax[t] + 1);
    int64_t* f = &info[8 * t];
    f[0] = rp[ra];
    f[1] = rp[rb] - rp[ra];
    f[2] = lo;
    f[3] = hi;
    f[4] = cmin[t];
    f[5] = cmax[t];
  }
  HIPC(ctx->d_tinfo.alloc(8 * nt));
  HIPC(hipMemcpy(ctx->d_tinfo, info.data(), 8 * nt * sizeof(int64_t), hipMemcpyHostToDevice));
  const int64_t grid = window_grid();
  ctx->tiles_per_wg = std::max<int64_t>(1, (nt + grid - 1) / grid);
  {
    // dense tiles of 16 x (16 + 2H) doubles pay when they stream no more than ~1.25x the
    // CSR's values + column indices (C4a: 18.4 KB vs 19.2 KB per tile)
    const int H = hneed <= 32 ? 32 : hneed <= 64 ? 64 : 0;
    const int NG = H ? (2 * H + 16) / 16 : 0;
    const double dense_bytes = (double)nt * 16.0 * 16.0 * NG * 8.0;
    if (H && dense_bytes <= 1.25 * 12.0 * (double)ctx->nnz) {
      const size_t elems = (size_t)bt_tile_slots(nt, ctx->tiles_per_wg) * NG * 256;
      HIPC(ctx->d_bt.alloc(elems));
      HIPC(hipMemsetAsync(ctx->d_bt, 0, elems * sizeof(double), ctx->stream));
      if (!ctx->d_zrow) {
        HIPC(ctx->d_zrow.alloc(64));
        HIPC(hipMemsetAsync(ctx->d_zrow, 0, 64 * sizeof(double), ctx->stream));
      }
      CsrDev A3 = csr(ctx);
      bt_fill(A3, H, NG, ctx->d_bt, ctx->stream);
      HIPC(hipGetLastError());
      HIPC(hipStreamSynchronize(ctx->stream));
      ctx->bt_ng = NG;
#ifdef RBL_VARIANTS
      // (variants build only) RBL_BT_PACK = 1: pack the tiles (zeros dropped; C4a: 13.1 KB per tile instead of
      // 18.4 KB, 3 GB less HBM at n = 1e7).  Off by default: the kernel is not bound by its
      // A bytes (one wave per SIMD, 60 % MFMA busy, fp64 MFMA and VALU do not co-issue) and
      // the index arithmetic of the packed loads costs more than the bytes save (3.56 vs
      // 3.40 ms per launch at C4a)
      const char* pk = getenv("RBL_BT_PACK");
      if (pk && atoi(pk) == 1) {
        const int64_t nslots = bt_tile_slots(nt, ctx->tiles_per_wg);
        HIPC(ctx->d_btp_hdr.alloc((size_t)nslots * bt_pack_words(NG)));
        int64_t nval = 0;
        double* pval = nullptr;
        const int prc = bt_pack(ctx->d_bt, nslots, NG, ctx->d_btp_hdr, &pval, &nval, ctx->stream);
        ctx->d_btp_val.adopt(pval);
        if (prc != 0) return prc == (int)hipErrorOutOfMemory ? RBL_ERR_OOM : RBL_ERR_HIP;
        ctx->d_bt.reset();
      } else {
        // A symmetric (bit for bit, as Lanczos assumes): store the diagonal group and the
        // right strip only — 10 of 18.4 KB per tile at H = 64; the kernel transposes the left
        // groups back from the previous tiles' strips (same U bits).  Opt-in (RBL_BT_HALF = 1)
        // while it measures slower than the whole tiles.
        const char* hf = getenv("RBL_BT_HALF");
        if (hf && atoi(hf) == 1) {
          double *half = nullptr, *edge = nullptr;
          const int hrc = bt_half(ctx->d_bt, nt, ctx->tiles_per_wg, NG, &half, &edge, ctx->stream);
          if (hrc > 0) return hrc == (int)hipErrorOutOfMemory ? RBL_ERR_OOM : RBL_ERR_HIP;
          if (hrc == 0) {
            ctx->d_bt.reset();
            ctx->d_bth.adopt(half);
            ctx->d_bte.adopt(edge);
          }
        }
      }
#endif
    }
  }
  // column-panel SpMM (spmm_panel.hip; not when the band tiles serve the matrix): per block of
  // R = 64 rpg rows the panels its columns span and every row's count in each of them;
  // applicable when no block spans more than kPanelMax panels (a window of 16 K rows: beyond
  // that the panels' re-reads cost more than the gathers they replace)
  if (!ctx->bt_ng) {
    const int pw = panel_width();
    // 8 rows per group (16-entry chunks) when a row's count per panel is mostly small, else 4
    // (32-entry chunks): the mean count per row and panel at 512-row blocks decides
    auto plan = [&](int R, std::vector<int32_t>* bp, int64_t* maxp, int64_t* staged) {
      const int tpb = R / kWindowTileRows;
      const int64_t nb = (nt + tpb - 1) / tpb;
      if (bp) bp->assign(4 * nb, 0);
      *maxp = *staged = 0;
      int64_t coff = 0;
      for (int64_t bk = 0; bk < nb; ++bk) {
        int64_t lo = INT64_MAX, hi = -1;
        for (int64_t t = bk * tpb; t < std::min(nt, (bk + 1) * tpb); ++t) {
          lo = std::min(lo, cmin[t]);
          hi = std::max(hi, cmax[t]);
        }
        const int64_t np = hi / pw - lo / pw + 1;
        if (bp) {
          (*bp)[4 * bk] = (int32_t)(lo / pw);
          (*bp)[4 * bk + 1] = (int32_t)(hi / pw);
          (*bp)[4 * bk + 2] = (int32_t)(uint32_t)(coff & 0xffffffff);
          (*bp)[4 * bk + 3] = (int32_t)(coff >> 32);
        }
        coff += np * R;
        *maxp = std::max(*maxp, np);
        *staged += np * pw;
      }
      return nb;
    };
    int64_t maxp = 0, staged = 0;
    plan(512, nullptr, &maxp, &staged);
    // the kernel's shape by the mean count per row and panel at 512-row blocks: 8 rows per
    // group with 16-record chunks up to a mean of 16, else 4 rows per group with 48-record
    // chunks (the three shapes forced at H = 128..2048: profiles/r06_panel_shapes_b30.txt)
    const double mean_cnt = (double)ctx->nnz / std::max(1.0, (double)(staged / pw) * 512);
#ifdef RBL_PANEL_RPG  // (probe builds: tools/build_variant.sh-style A/B of the kernel shape)
    const int rpg = RBL_PANEL_RPG, pch = RBL_PANEL_CH;
#else
    const int rpg = mean_cnt <= 16.0 ? 8 : 4;
    const int pch = rpg == 8 ? 16 : 48;
#endif
    const int R = 64 * rpg;
    std::vector<int32_t> bp;
    const int64_t nb = plan(R, &bp, &maxp, &staged);
    const int64_t ncnt = bp.empty() ? 0 : ((int64_t)(uint32_t)bp[4 * nb - 2] | ((int64_t)bp[4 * nb - 1] << 32)) +
                                              ((int64_t)bp[4 * nb - 3] - bp[4 * nb - 4] + 1) * R;
    // the kernel addresses a block's records with 32-bit buffer offsets: every block's
    // values within 2 GiB (the block bases, rowptr[b R], read strided)
    int64_t maxblk = 0;
    if (maxp <= kPanelMax && ctx->n / pw < INT32_MAX && nb > 0) {
      std::vector<int64_t> zb(nb + 1);
      HIPC(hipMemcpy2D(zb.data(), sizeof(int64_t), ctx->d_rowptr, (size_t)R * sizeof(int64_t),
                       sizeof(int64_t), (size_t)nb, hipMemcpyDeviceToHost));
      zb[nb] = ctx->nnz;
      for (int64_t bk = 0; bk < nb; ++bk) maxblk = std::max(maxblk, zb[bk + 1] - zb[bk]);
    }
    bool fits = maxp <= kPanelMax && ctx->n / pw < INT32_MAX && nb > 0 && maxblk * 8 < INT32_MAX;
    // the records are a second copy of the matrix: without room for it, no panels (the gathers).
    // An allocation that fails here is not an error: this rank just runs another kernel (the
    // several-rank setup after this is collective, so no rank may leave before it)
    if (fits) {
      const bool ok =
          ctx->d_panel_val.alloc(std::max<int64_t>(ctx->nnz, 1)) == hipSuccess &&
          ctx->d_panel_col.alloc(std::max<int64_t>(ctx->nnz, 1)) == hipSuccess &&
          ctx->d_panel_blk.alloc(4 * nb) == hipSuccess &&
          ctx->d_panel_cnt.alloc(std::max<int64_t>(ncnt, 1)) == hipSuccess &&
          ctx->d_panel_st.alloc(std::max<int64_t>(ncnt, 1)) == hipSuccess;
      if (!ok) {
        (void)hipGetLastError();
        free_panels(ctx);
        fits = false;
      }
    }
    if (fits) {
      HIPC(hipMemcpy(ctx->d_panel_blk, bp.data(), 4 * nb * sizeof(int32_t), hipMemcpyHostToDevice));
      CsrDev A2 = csr(ctx);
      if (panel_format(A2, ctx->d_panel_blk, R, nb, ctx->d_panel_cnt, ctx->d_panel_st, ncnt,
                       ctx->d_panel_col, ctx->d_panel_val, ctx->stream) != 0)
        return fail(ctx, RBL_ERR_HIP, "panel_format");
      HIPC(hipStreamSynchronize(ctx->stream));
      ctx->panel_nblk = nb;
      ctx->panel_rpg = rpg;
      ctx->panel_ch = pch;
      // by default only where the panels pay: a staged Q row read >= 4 times from LDS on
      // average (bands; a scattered pattern's blocks span the whole matrix: the gathers).  Ahead
      // of the LDS-window kernel where both apply: 5.0 vs 7.6 ms at H = 72 and 96, n = 1e7
      // (profiles/r06_panel_vs_window_b19.txt)
      ctx->panel_auto = 4 * staged <= ctx->nnz;
      ctx->panel_span = maxp * pw;
      if (!ctx->d_zrow) {  // the panel rows outside the Q range read it
        HIPC(ctx->d_zrow.alloc(64));
        HIPC(hipMemset(ctx->d_zrow, 0, 64 * sizeof(double)));
      }
    }
  }
  if (!ctx->keep_csr && ctx->bt_ng) {
    // RBL_OPT_KEEP_CSR = 0: the band tiles are the matrix from here on
    ctx->d_col.reset();
    ctx->d_val.reset();
    static_cast<SegTableBufs&>(*ctx) = SegTableBufs{};
    ctx->seg_ntasks = ctx->seg_nlong = 0;
    free_tiers(ctx);
    ctx->window_ok16 = ctx->window_ok32 = false;
    ctx->band_ok16 = ctx->band_ok32 = false;
    ctx->band_gram = ctx->band_pair = false;
    ctx->csr_dropped = true;
    return RBL_OK;
  }
  if (ctx->band_ok16 || ctx->band_ok32) {  // dense-tile positions for the band kernel
    HIPC(ctx->d_bpos.alloc(ctx->nnz + kCsrPad));
    HIPC(hipMemsetAsync(ctx->d_bpos + ctx->nnz, 0, kCsrPad * sizeof(uint16_t), ctx->stream));
    CsrDev A2 = csr(ctx);
    band_positions(A2, ctx->d_bpos, ctx->stream);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  return RBL_OK;
}

// ---- timers --------------------------------------------------------------------------
hipEvent_t next_event(rbl_ctx* ctx) {
  if (ctx->ev_used == ctx->ev_pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    ctx->ev_pool.push_back(e);
  }
  return ctx->ev_pool[ctx->ev_used++];
}
struct StageScope {
  rbl_ctx* ctx;
  int stage;
  hipEvent_t a = nullptr;
  // every stage is also a roctx range named like the reference's TimerOutputs labels
  // (RBL_gpu.jl:152-187: "AQ", "3-term", ...): `rocprofv3 --marker-trace` shows them
  hipStream_t st;
  int parent = -1;
  StageScope(rbl_ctx* c, int s, hipStream_t on = nullptr) : ctx(c), stage(s), st(on ? on : c->stream) {
    roctxRangePushA(kStageNames[s]);
    if (ctx->timers == 1 ||
        (ctx->timers == 2 && (s == RBL_STAGE_AQ || s == RBL_STAGE_PART_REORTH))) {
      a = next_event(ctx);
      if (a) hipEventRecord(a, st);
    }
    // a collective issued inside another stage on the same stream: its span is "comm" only, so
    // the stages of a step sum to the step's stream time (the multi-rank line's per-rank split)
    if (s == RBL_STAGE_COMM)
      for (auto it = ctx->open_stages.rbegin(); it != ctx->open_stages.rend(); ++it)
        if (it->st == st) {
          parent = it->stage;
          break;
        }
    ctx->open_stages.push_back({s, st});
  }
  ~StageScope() {
    ctx->open_stages.pop_back();
    if (a) {
      hipEvent_t b = next_event(ctx);
      if (b) {
        hipEventRecord(b, st);
        ctx->marks.push_back({stage, a, b, parent});
      }
    }
    roctxRangePop();
  }
};
void harvest_timers(rbl_ctx* ctx) {
  // stages whose end event has completed; the rest (steps still running after an rbl_fetch
  // that waited only for earlier steps) stay for a later harvest, their events in use
  std::vector<rbl_ctx::Mark> keep;
  for (auto& m : ctx->marks) {
    if (hipEventQuery(m.b) != hipSuccess) {
      keep.push_back(m);
      continue;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, m.a, m.b) == hipSuccess) {
      if (m.stage < RBL_NUM_STAGES) {
        ctx->stage_ms[m.stage] += ms;
        if (m.parent >= 0) ctx->stage_ms[m.parent] -= ms;  // (recorded whenever the child is)
      } else {
        ctx->comm_dev_ms[m.stage - RBL_NUM_STAGES] += ms;  // a CollScope's span
      }
    }
  }
  ctx->marks.swap(keep);
  if (ctx->marks.empty()) ctx->ev_used = 0;
}

// ---- collectives ---------------------------------------------------------------------
// One collective call: the host wall time inside the transport (RCCL enqueues and returns;
// the shm / in-process stand-ins block) and, while the full stage timers run, a hipEvent pair
// around it on its stream — the span the collective holds that stream, waiting for the peers
// included.  Read per rank through rbl_comm_stats (RBL_COMM_*_HOST_NS / *_DEV_NS).
struct CollScope {
  rbl_ctx* ctx;
  int kind;  // 0 all-reduce, 1 exchange
  hipStream_t st;
  hipEvent_t a = nullptr;
  std::chrono::steady_clock::time_point t0;
  CollScope(rbl_ctx* c, int k, hipStream_t on) : ctx(c), kind(k), st(on) {
    if (ctx->timers == 1) {
      a = next_event(ctx);
      if (a) hipEventRecord(a, st);
    }
    t0 = std::chrono::steady_clock::now();
  }
  ~CollScope() {
    ctx->comm_host_ns[kind] += std::chrono::duration_cast<std::chrono::nanoseconds>(
                                   std::chrono::steady_clock::now() - t0).count();
    if (a) {
      hipEvent_t b = next_event(ctx);
      if (b) {
        hipEventRecord(b, st);
        ctx->marks.push_back({RBL_NUM_STAGES + kind, a, b});
      }
    }
  }
};

int allreduce(rbl_ctx* ctx, double* buf, size_t count) {
  if (ctx->nranks == 1) return RBL_OK;
  StageScope t(ctx, RBL_STAGE_COMM);
  CollScope c(ctx, 0, ctx->stream);
  COMMC(ctx->comm->allreduce_sum(buf, count, ctx->stream, &ctx->err));
  ctx->comm_stats[RBL_COMM_ALLREDUCE_CALLS] += 1;
  ctx->comm_stats[RBL_COMM_ALLREDUCE_BYTES] += (int64_t)(count * sizeof(double));
  return RBL_OK;
}

void count_exchange(rbl_ctx* ctx, const std::vector<Comm::Xfer>& x) {
  ctx->comm_stats[RBL_COMM_EXCHANGE_CALLS] += 1;
  for (const auto& t : x) {
    ctx->comm_stats[RBL_COMM_SEND_BYTES] += (int64_t)(t.nsend * sizeof(double));
    ctx->comm_stats[RBL_COMM_RECV_BYTES] += (int64_t)(t.nrecv * sizeof(double));
  }
}

// a step's grouped halo send/recv on `st`, timed and counted
int exchange(rbl_ctx* ctx, const std::vector<Comm::Xfer>& x, hipStream_t st) {
  CollScope c(ctx, 1, st);
  COMMC(ctx->comm->exchange(x, st, &ctx->err));
  count_exchange(ctx, x);
  return RBL_OK;
}

// Gram C = W^T X over all ranks.  C layout [nW*w][X.count*X.w].  (comm = false: this rank's
// share only, for a caller that all-reduces it together with another buffer)
int gram(rbl_ctx* ctx, const PanelRun& W, const Panels& X, double* C, const int* skip, bool comm = true) {
  const int xcols = X.count * X.w;
  const int splits = gram_splits(ctx->nloc, W.count, W.w, xcols);
  const int64_t len = (int64_t)W.count * W.w * xcols;
  if ((size_t)splits * len > ctx->slab_elems)
    return fail(ctx, RBL_ERR_INVALID, "internal: Gram slab too small");
  if (ctx->nloc > 0) {
    gram_partial(ctx->nloc, W, X, ctx->d_slab, splits, skip, ctx->stream);
    reduce_slab(ctx->d_slab, splits, len, C, skip, ctx->stream);
  } else {
    HIPC(hipMemsetAsync(C, 0, len * sizeof(double), ctx->stream));
  }
  HIPC(hipGetLastError());
  return comm ? allreduce(ctx, C, (size_t)len) : RBL_OK;
}

PanelRun run1(const double* p, int w) {
  PanelRun r;
  r.base = p;
  r.stride = 0;
  r.count = 1;
  r.w = w;
  return r;
}
Panels pan1(const double* p, int w) {
  Panels x;
  x.ptr[0] = p;
  x.count = 1;
  x.w = w;
  return x;
}
Panels pan2(const double* p0, const double* p1, int w) {
  Panels x;
  x.ptr[0] = p0;
  x.ptr[1] = p1;
  x.count = 2;
  x.w = w;
  return x;
}

// small-buffer carve (b x b each)
// S_CHS*: chol scratch (b > 64); S_RINV1: R1^-1 kept for the 3-pass CholQR; S_CLOC: the next
// step's local-reorth Gram
// (S_CLOC follows S_G: CholQR's pass-3 Gram and the next step's local-reorth Gram share one
// all-reduce of 2 b^2)
// S_CX precedes S_G: with RBL_OPT_CLOC_DERIVE the pass-3 Gram travels with the direct cross Gram
// of an ill-conditioned step instead (tsqr), while S_CLOC holds the derived coefficient
enum { S_R = 0, S_RINV, S_RTOT, S_BPREV, S_AI, S_CX, S_G, S_CLOC, S_BT, S_CHS0, S_CHS1, S_RINV1, S_NSMALL };
static_assert(S_CLOC == S_G + 1, "tsqr all-reduces [S_G | S_CLOC] as one 2 b^2 buffer");
static_assert(S_G == S_CX + 1, "tsqr all-reduces [S_CX | S_G] as one 2 b^2 buffer");
double* smallp(rbl_ctx* ctx, int which) { return ctx->d_small + (int64_t)which * ctx->b * ctx->b; }

int tsmm_checked(rbl_ctx* ctx, const PanelRun& X, const double* C, int ldc, const Panels& Y,
                 double alpha, double beta, const int* skip, double* xslab = nullptr,
                 int* xgrid = nullptr) {
  if (xgrid) *xgrid = 0;
  if (ctx->nloc <= 0) return RBL_OK;
  tsmm(ctx->nloc, X, C, ldc, Y, alpha, beta, skip, ctx->stream, xslab, xgrid);
  HIPC(hipGetLastError());
  return RBL_OK;
}

// Fused one-pass row operation (rowop.hip): Y = beta Y + alpha X C and, if G, the Gram
// G = Y^T Y over all ranks.  b in {16, 32}.
int rowop(rbl_ctx* ctx, const double* X, const double* C, double* Y, double alpha, double beta,
          double* G, const int* skip, const float* X32 = nullptr, float* Y32 = nullptr,
          const int* f64flag = nullptr, bool tri = false) {
  const int b = ctx->b;
  const int grid = rowgram_grid(ctx->nloc);
  if (G && (size_t)grid * b * b > ctx->slab_elems)
    return fail(ctx, RBL_ERR_INVALID, "internal: row-op slab too small");
  if (ctx->nloc > 0) {
    // without a Gram the grid follows the kernel's occupancy (no partials to count)
    rowgram(ctx->nloc, b, X, C, b, Y, alpha, beta, G ? ctx->d_slab : nullptr, G ? grid : 0, skip,
            ctx->stream, X32, Y32, f64flag, tri && !X32);
    HIPC(hipGetLastError());
  } else if (G) {  // no rows on this rank: its share of the Gram is zero (the all-reduce still runs)
    HIPC(hipMemsetAsync(ctx->d_slab, 0, (size_t)grid * b * b * sizeof(double), ctx->stream));
  }
  if (!G) return RBL_OK;
  reduce_slab(ctx->d_slab, grid, (int64_t)b * b, G, skip, ctx->stream);
  HIPC(hipGetLastError());
  return allreduce(ctx, G, (size_t)b * b);
}

// Gram slab of a run (doubles): the largest Gram is the partial-reorth one, (max_blocks-1)
// panels x 2b per split; also the row ops' partials, the partial-reorth update's local-reorth
// Gram partials and the fp32 Grams.  rbl_start allocates it; the automatic device-block plan
// (RBL_OPT_DEVICE_BLOCKS < 0) budgets it — one formula for both.
size_t gram_slab_elems(const rbl_ctx* ctx, int b, int max_blocks, int basis_bits) {
  size_t slab = 0;
  for (int nW = 1; nW <= std::max(1, max_blocks - 1); ++nW)
    for (int xc : {b, 2 * b}) {
      const size_t sp = (size_t)gram_splits(ctx->nloc, nW, b, xc);
      slab = std::max(slab, sp * nW * b * xc);
    }
  slab = std::max(slab, (size_t)2 * rowgram_grid(ctx->nloc, kRowgramMaxPerCu) * b * b);  // rowop partials (+ cross Gram)
  // the partial-reorth update's local-reorth Gram partials (one b x b per 128-row tile:
  // n_local b^2 / 128 doubles, a quarter of a block at b = 32)
  if (b == 32 && basis_bits == 64 && (ctx->fuse & 2)) {
    const int xg = tsmm44_xg_grid(ctx->nloc);
    slab = std::max(slab, (size_t)(xg + reduce_scratch_splits(xg)) * b * b);
  }
  if (basis_bits == 32)  // fp32 Grams: up to (max_blocks-1) panels x 2b per split
    slab = std::max(slab, (size_t)gram32_splits(ctx->nloc) * std::max(1, max_blocks - 1) * b * 2 * b);
  return slab;
}

bool has_matrix(const rbl_ctx* ctx) { return ctx->d_rowptr || ctx->dense || ctx->rect || ctx->kernop; }

// the kernel matrix held as kernelop.hip takes it
static_assert(RBL_KERNEL_RBF == kKernRbf && RBL_KERNEL_LAPLACE == kKernLaplace && RBL_KERNEL_POLY == kKernPoly &&
                  RBL_KERNOP_MAX_DIM == kKernMaxDim,
              "rbl_hip.h and kernels.hpp name the same kernels");
KernOp kernop(const rbl_ctx* ctx) {
  KernOp op;
  op.n = ctx->n;
  op.d4 = ctx->kern_d4;
  op.kind = ctx->kern_kind;
  op.degree = ctx->kern_degree;
  op.gamma = ctx->kern_gamma;
  op.coef0 = ctx->kern_coef0;
  op.nugget = ctx->kern_nugget;
  op.X = ctx->d_kern_x;
  op.nrm = ctx->d_kern_nrm;
  op.scale = ctx->d_kern_scale;
  return op;
}

// one orientation of a rectangular B as the kernels take it (0: B's rows, 1: B^T's rows)
CsrDev::Tier rect_tier(const rbl_ctx* ctx, int side) {
  const auto& T = ctx->rect_side[side];
  CsrDev::Tier D;
  D.rowptr = T.rowptr;
  D.col = T.col;
  D.val = T.val;
  D.ntasks = T.ntasks;
  D.nlong = T.nlong;
  D.trow = T.trow;
  D.tinfo = T.tinfo;
  D.slot_k0 = T.slot_k0;
  D.lrow = T.lrow;
  D.lslot = T.lslot;
  D.scratch = T.scratch;
  return D;
}
// the m x b work block Y = B Q_i of the normal operator, and with a shift set the small buffers
// of its two reductions (t, s: b doubles each; the workgroup partials of the larger side)
int ensure_rect_y(rbl_ctx* ctx, int b) {
  if (!ctx->d_rect_y || ctx->rect_y_cols < b) {
    HIPC(hipStreamSynchronize(ctx->stream));
    ctx->d_rect_y.reset();
    ctx->rect_y_cols = 0;
    HIPC(ctx->d_rect_y.alloc((size_t)ctx->rect_m * b));
    ctx->rect_y_cols = b;
  }
  if (ctx->rect_shift && ctx->rect_ts_cols < b) {
    HIPC(hipStreamSynchronize(ctx->stream));
    ctx->d_rect_ts.reset();
    ctx->d_rect_part.reset();
    ctx->rect_ts_cols = 0;
    const size_t grid = (size_t)rect_colsum_grid(std::max(ctx->rect_m, ctx->n), b);
    HIPC(ctx->d_rect_ts.alloc((size_t)2 * b));
    HIPC(ctx->d_rect_part.alloc(grid * b));
    ctx->rect_ts_cols = b;
  }
  return RBL_OK;
}

// fp32 basis: the band-tile SpMM and the 3-term update read the fp32 blocks directly
bool direct32_ok(const rbl_ctx* ctx, int b) {
  return !ctx->dense && (ctx->spmm_variant == 0 || ctx->spmm_variant == 4) && (b == 32 || b == 16) &&
         (ctx->bt_ng == 5 || ctx->bt_ng == 9);
}
// the fp64 scratch block of the fp32 path (widened Q_{i-1}, Ritz / get_block widening),
// allocated on first use when the direct path made it unnecessary at rbl_start
int ensure_qm64(rbl_ctx* ctx) {
  if (ctx->d_Qm64) return RBL_OK;
  HIPC(ctx->d_Qm64.alloc((std::max<int64_t>(ctx->nloc, 1) + kRowPad) * ctx->b));
  return RBL_OK;
}

// The indexed halo serves only the segmented gather's own / halo column tiers (b in {16, 32});
// any other SpMM (another b, a kernel pinned by RBL_OPT_SPMM_KERNEL) reads the range halo,
// which is kept beside it.  The rule depends only on state every rank shares (the collective
// `ghost` decision, b, the option), so all ranks pick the same exchange for a call.
bool use_ghost(const rbl_ctx* ctx, int b) {
  return ctx->ghost && ctx->nranks > 1 && (b == 16 || b == 32) &&
         (ctx->spmm_variant == 0 || ctx->spmm_variant == 5);
}
// rows of the halo buffer for block size b: the ghost slots, or the range [ext_lo, ext_hi)
int64_t qext_rows(const rbl_ctx* ctx, int b) {
  return std::max<int64_t>(use_ghost(ctx, b) ? ctx->n_ghost : ctx->ext_hi - ctx->ext_lo, 1);
}
// grow the halo buffer (zeroed: rows between the received ranges stay finite) for block size b
int ensure_qext(rbl_ctx* ctx, int b, hipStream_t st) {
  const size_t need = (size_t)qext_rows(ctx, b) * b;
  if (ctx->d_qext && ctx->qext_cap >= need) return RBL_OK;
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->d_qext.reset();
  ctx->qext_cap = 0;
  HIPC(ctx->d_qext.alloc(need));
  HIPC(hipMemsetAsync(ctx->d_qext, 0, need * sizeof(double), st));
  ctx->qext_cap = need;
  return RBL_OK;
}

// U = A Qin (+ U -= Qprev Bi^T when Qprev): the SpMM of RBL_gpu.jl:176-177, or for a dense
// A (RBL_gpu.jl:205 with A::Matrix) the panel GEMM on fp64 MFMA (tsmm44 over the panels of
// the local rows, Q gathered to all n rows by the halo exchange).  Returns the number of
// A_i partials the band kernel formed in `slab` (0: none), or a negative status.
// This is the stored matrix alone; apply_A below adds the low-rank update when one is set.
int apply_A_stored(rbl_ctx* ctx, const double* Qin, int64_t off, int b, double* U, const double* Qprev,
                   const double* Bi, double* slab, const double* qloc, const double* lfix_c,
                   double* lfix_q, int64_t lf_lo, int64_t lf_hi, hipEvent_t seg_wait) {
  if (ctx->nloc <= 0) return 0;
  if (ctx->rect) {  // B^T (B Q_i): two gather passes, the 3-term epilogue fused into the second
    CHK(ensure_rect_y(ctx, b));
    const double* Q = Qin + (0 - off) * b;
    if (ctx->rect_shift) {
      // C^T (C Q_i), C = B - u v^T:  t = Q^T v,  Y = B Q - u t^T,  s = Y^T u,
      // U = B^T Y - v s^T (- Q_{i-1} B_i^T) — all in stream order, t and s never leave the device
      double *t = ctx->d_rect_ts, *sv = ctx->d_rect_ts + b;
      rect_colsum(ctx->n, b, ctx->d_shift_v, Q, ctx->d_rect_part, t, ctx->stream);
      spmm_rect(rect_tier(ctx, 0), Q, b, ctx->d_rect_y, nullptr, nullptr, nullptr, ctx->stream,
                ctx->d_shift_u, t);
      rect_colsum(ctx->rect_m, b, ctx->d_shift_u, ctx->d_rect_y, ctx->d_rect_part, sv, ctx->stream);
      spmm_rect(rect_tier(ctx, 1), ctx->d_rect_y, b, U, Qprev, Bi, nullptr, ctx->stream,
                ctx->d_shift_v, sv);
      ctx->path_stats[RBL_PATH_SPMM] += 1;
      return 0;
    }
    spmm_rect(rect_tier(ctx, 0), Q, b, ctx->d_rect_y, nullptr, nullptr, nullptr, ctx->stream);
    spmm_rect(rect_tier(ctx, 1), ctx->d_rect_y, b, U, Qprev, Bi, nullptr, ctx->stream);
    ctx->path_stats[RBL_PATH_SPMM] += 1;
    return 0;
  }
  if (ctx->kernop) {  // K evaluated tile by tile from the points; the 3-term term as for a dense A
    if (!kernop_apply(kernop(ctx), Qin + (0 - off) * b, b, U, ctx->stream))
      return fail(ctx, RBL_ERR_INVALID, "internal: kernel-matrix apply: shape not served");
    if (Qprev) {
      transpose_small(Bi, smallp(ctx, S_BT), b, ctx->stream);
      CHK(tsmm_checked(ctx, run1(Qprev, b), smallp(ctx, S_BT), b, pan1(U, b), -1.0, 1.0, nullptr));
    }
    return 0;
  }
  if (ctx->csr_dropped && rbl_spmm_kernel_for(ctx, b) != 5)
    return fail(ctx, RBL_ERR_STATE, "the CSR was released (RBL_OPT_KEEP_CSR = 0): only the band-tile "
                                    "SpMM (b in {16, 32}) can run");
  if (!ctx->dense) {
    CsrDev A = csr(ctx);
    // indexed halo: the own-column tier always reads the block the exchange sent from (a rank
    // without nonzeros runs the plain gather, which reads no Q row at all)
    if (!qloc && ctx->ghost_active && ctx->nranks > 1 && rbl_spmm_kernel_for(ctx, b) == 6)
      qloc = ctx->ghost_local;
    if (qloc) {  // own rows from the block itself (halo_exchange without the local copy)
      A.qloc = qloc;
      A.loc_lo = ctx->r0;
      A.loc_hi = ctx->r0 + ctx->nloc;
    }
    A.seg_wait = seg_wait;  // own/halo column tiers: the halo tier waits for the exchange
    int two_wave = 0;
    A.two_wave = &two_wave;
    if (lfix_c) {  // local reorth fused into the SpMM's staging (RBL_OPT_FUSE bit 2)
      A.lfix_c = lfix_c;
      A.lfix_q = lfix_q;
      A.lfix_lo = lf_lo;
      A.lfix_hi = lf_hi;
    }
    const int parts = spmm(A, Qin, off, b, U, Qprev, Bi, ctx->spmm_variant, ctx->stream, slab);
    if (parts < 0) return fail(ctx, RBL_ERR_INVALID, "internal: split-source SpMM needs the band-tile kernel");
    ctx->path_stats[RBL_PATH_SPMM] += 1;
    ctx->path_stats[RBL_PATH_SPMM_TWO_WAVE] += two_wave;
    if (lfix_c) {
      ctx->path_stats[RBL_PATH_SPMM_LOC_FUSED] += 1;
      ctx->path_stats[RBL_PATH_LOCFIX_REST] += 1;
      StageScope t(ctx, RBL_STAGE_LOC_REORTH);
      spmm_bt_locfix_rest(A, lfix_q, Qprev, lfix_c, ctx->stream);
    }
    return parts;
  }
  if (b > ctx->qfull_cols) {  // Q gathered to all n rows, zero-padded to 32 * dense_panels
    ctx->d_qfull.reset();
    ctx->qfull_cols = 0;
    HIPC(ctx->d_qfull.alloc((size_t)ctx->dense_panels * 32 * b));
    HIPC(hipMemsetAsync(ctx->d_qfull, 0, (size_t)ctx->dense_panels * 32 * b * sizeof(double), ctx->stream));
    ctx->qfull_cols = b;
  }
  HIPC(hipMemcpyAsync(ctx->d_qfull, Qin + (0 - off) * b, ctx->n * b * sizeof(double),
                      hipMemcpyDeviceToDevice, ctx->stream));
  PanelRun X;
  X.base = ctx->d_dense;
  X.stride = ctx->nloc * 32;
  X.w = 32;
  X.count = (int)ctx->dense_panels;
  CHK(tsmm_checked(ctx, X, ctx->d_qfull, b, pan1(U, b), 1.0, 0.0, nullptr));
  if (Qprev) {
    transpose_small(Bi, smallp(ctx, S_BT), b, ctx->stream);
    CHK(tsmm_checked(ctx, run1(Qprev, b), smallp(ctx, S_BT), b, pan1(U, b), -1.0, 1.0, nullptr));
  }
  return 0;
}

// the small buffers of the low-rank update for block size b: w and c (lr_rp x b each) and the
// workgroup partials of w
int ensure_lr_bufs(rbl_ctx* ctx, int b) {
  if (ctx->d_lr_wc && ctx->lr_cols >= b) return RBL_OK;
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->d_lr_wc.reset();
  ctx->d_lr_part.reset();
  ctx->lr_cols = 0;
  const size_t grid = (size_t)lr_project_grid(ctx->nloc, b, ctx->lr_rp);
  HIPC(ctx->d_lr_wc.alloc((size_t)2 * ctx->lr_rp * b));
  HIPC(ctx->d_lr_part.alloc(grid * ctx->lr_rp * b));
  ctx->lr_cols = b;
  return RBL_OK;
}

// U = Op Qin (- Qprev Bi^T), Op = A or, with an update set (rbl_set_lowrank), A + P S P^T: every
// n-sized product of the library goes through here (rbl_apply, the block step, the Chebyshev
// recurrences, the moment pass, the Ritz projection's W = Op V), so each sees the same operator.
// The update runs in stream order after the SpMM, its fused 3-term epilogue and — with the local
// reorth fused into the SpMM's staging — spmm_bt_locfix_rest, so the projection reads the final
// Q_i:  w = P^T Q_i,  c = S w,  U[row, :] += P[row, :] c  for row < n_local (the kRowPad spare rows
// stay as the SpMM left them).  The band kernel's A_i partials are Q_i^T U of the U before the
// update: with an update set 0 is returned (and no partials are asked for unless the fused local
// reorth needs that kernel), so the caller's Gram forms A_i from the final U.
int apply_A(rbl_ctx* ctx, const double* Qin, int64_t off, int b, double* U, const double* Qprev,
            const double* Bi, double* slab, const double* qloc = nullptr,
            const double* lfix_c = nullptr, double* lfix_q = nullptr, int64_t lf_lo = 0,
            int64_t lf_hi = 0, hipEvent_t seg_wait = nullptr) {
  if (ctx->lr_r == 0 || ctx->nloc <= 0)
    return apply_A_stored(ctx, Qin, off, b, U, Qprev, Bi, slab, qloc, lfix_c, lfix_q, lf_lo, lf_hi,
                          seg_wait);
  if (ctx->nranks > 1 || ctx->rect)
    return fail(ctx, RBL_ERR_STATE, "internal: a low-rank update needs one rank and a square A");
  CHK(ensure_lr_bufs(ctx, b));
  const int parts = apply_A_stored(ctx, Qin, off, b, U, Qprev, Bi, lfix_c ? slab : nullptr, qloc,
                                   lfix_c, lfix_q, lf_lo, lf_hi, seg_wait);
  if (parts < 0) return parts;
  const double* X = Qin + (ctx->r0 - off) * b;  // the local rows of Q_i (one rank: the block)
  double *w = ctx->d_lr_wc, *c = ctx->d_lr_wc + (size_t)ctx->lr_rp * b;
  lr_project(ctx->nloc, b, ctx->lr_rp, ctx->d_lr_P, X, ctx->d_lr_part, w, ctx->stream);
  lr_small(ctx->lr_r, ctx->lr_rp, b, ctx->d_lr_S, w, c, ctx->stream);
  lr_update(ctx->nloc, b, ctx->lr_rp, ctx->d_lr_P, c, U, ctx->stream);
  return 0;
}

// The two work blocks of the filter recurrence for block size b (allocated and zeroed like d_U:
// the band kernels store unguarded into the kRowPad spare rows).
// A series (rbl_set_filter_series) rotates through a third block, allocated only while one is set.
bool has_series(const rbl_ctx* ctx) { return !ctx->ser_mu.empty(); }
bool has_filter(const rbl_ctx* ctx) { return ctx->filt_deg > 0 || has_series(ctx); }

int ensure_filter_bufs(rbl_ctx* ctx, int b) {
  const int want = has_series(ctx) ? 3 : 2;
  if (ctx->d_filt[0] && ctx->d_filt[1] && ctx->filt_cols >= b) {
    if (want == 2 || ctx->d_filt[2]) return RBL_OK;
    // the two blocks of an earlier filter stay; the series' third joins them at their width
    const size_t len = (size_t)(std::max<int64_t>(ctx->nloc, 1) + kRowPad) * ctx->filt_cols;
    HIPC(ctx->d_filt[2].alloc(len));
    HIPC(hipMemsetAsync(ctx->d_filt[2], 0, len * sizeof(double), ctx->stream));
    return RBL_OK;
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  const size_t len = (size_t)(std::max<int64_t>(ctx->nloc, 1) + kRowPad) * b;
  for (auto& p : ctx->d_filt) p.reset();
  ctx->filt_cols = 0;
  for (int q = 0; q < want; ++q) {
    HIPC(ctx->d_filt[q].alloc(len));
    HIPC(hipMemsetAsync(ctx->d_filt[q], 0, len * sizeof(double), ctx->stream));
  }
  ctx->filt_cols = b;
  return RBL_OK;
}

// Per-term scalars of the scaled Chebyshev recurrence (Zhou & Saad): Y_j = al A Y_{j-1} +
// be Y_{j-1} + ga Y_{j-2} (rbl.filtered.cheb_scalars is the same arithmetic on the host).
struct ChebTerm { double al, be, ga; };
std::vector<ChebTerm> cheb_terms(int degree, double lo, double hi, double ref) {
  const double c = 0.5 * (lo + hi), e = 0.5 * (hi - lo);
  const double s1 = e / (ref - c);
  std::vector<ChebTerm> t;
  t.push_back({s1 / e, -(s1 / e) * c, 0.0});
  double sg = s1;
  for (int j = 2; j <= degree; ++j) {
    const double sn = 1.0 / (2.0 / s1 - sg);
    t.push_back({2.0 * sn / e, -(2.0 * sn / e) * c, -sg * sn});
    sg = sn;
  }
  return t;
}

// out = p(A) X (rbl_set_filter), one rank: X, out and the work blocks F0, F1 are distinct
// n_local x b row-major blocks; out, F0, F1 carry the kRowPad spare rows.  X is only read.
// Term j's SpMM writes W = A Y_{j-1} into the block that held Y_{j-3} (dead by then), and the
// row pass turns it into Y_j in place; the rotation starts so that Y_degree lands in `out`.
int cheb_apply(rbl_ctx* ctx, const double* X, int b, double* out, double* F0, double* F1) {
  if (ctx->nloc <= 0) return RBL_OK;
  const std::vector<ChebTerm> terms = cheb_terms(ctx->filt_deg, ctx->filt_lo, ctx->filt_hi, ctx->filt_ref);
  double* buf[3] = {out, F0, F1};
  const int d = ctx->filt_deg;
  const int shift = (3 - d % 3) % 3;  // Y_j lives in buf[(j + shift) % 3]; Y_d in buf[0]
  const double* y1 = X;        // Y_{j-1}
  const double* y2 = nullptr;  // Y_{j-2}
  const int64_t len = ctx->nloc * b;
  for (int j = 1; j <= d; ++j) {
    double* yj = buf[(j + shift) % 3];
    const int st = apply_A(ctx, y1, 0, b, yj, nullptr, nullptr, nullptr);
    if (st < 0) return st;
    const ChebTerm& t = terms[j - 1];
    cheb_axpby(len, yj, y1, j >= 2 ? y2 : nullptr, t.al, t.be, t.ga, yj, ctx->stream);
    HIPC(hipGetLastError());
    y2 = y1;
    y1 = yj;
  }
  return RBL_OK;
}

// out = sum_{j=0..d} mu_j T_j((A - cI)/e) X (rbl_set_filter_series), one rank: X, out and the
// work blocks F[0..2] are distinct n_local x b row-major blocks; F[] carry the kRowPad spare
// rows (the SpMMs write them), out is only streamed.  X is only read: it is T_0, so T_{j-1} of
// term 1 and T_{j-2} of term 2.  T_j lives in F[j % 3]: term j's SpMM writes W = A T_{j-1} into
// the block that held T_{j-3} (dead by then) and the fused pass turns W into T_j in place while
// it adds mu_j T_j to out; the first pass initialises out, the last stores no T_d.
int series_apply(rbl_ctx* ctx, const double* X, int b, double* out, const DevBuf<double> F[3]) {
  if (ctx->nloc <= 0) return RBL_OK;
  const std::vector<double>& mu = ctx->ser_mu;
  const int d = (int)mu.size() - 1;
  const double c = 0.5 * (ctx->ser_lo + ctx->ser_hi), e = 0.5 * (ctx->ser_hi - ctx->ser_lo);
  const double* t1 = X;        // T_{j-1}
  const double* t2 = nullptr;  // T_{j-2}
  const int64_t len = ctx->nloc * b;
  for (int j = 1; j <= d; ++j) {
    double* tj = F[j % 3];
    const int st = apply_A(ctx, t1, 0, b, tj, nullptr, nullptr, nullptr);
    if (st < 0) return st;
    const double al = (j == 1 ? 1.0 : 2.0) / e;
    cheb_series_term(len, tj, t1, t2, al, -al * c, mu[j], mu[0], tj, out, j == 1, j == d, ctx->stream);
    HIPC(hipGetLastError());
    t2 = t1;
    t1 = tj;
  }
  return RBL_OK;
}

// out = p(A) X with whichever filter is set (has_filter; the work blocks from ensure_filter_bufs)
int filter_apply(rbl_ctx* ctx, const double* X, int b, double* out, const DevBuf<double> F[3]) {
  if (has_series(ctx)) return series_apply(ctx, X, b, out, F);
  return cheb_apply(ctx, X, b, out, F[0], F[1]);
}

// RBL_OPT_UPD32: the fp32 route is taken for g <= tau (k_upd32_gate).  At 1/2 the fp32 route's
// column error is 1.1 .. 1.3x the fp64 route's (tests/test_upd32_host.py holds it to 8x, which a
// NumPy restatement reaches near g = 4); a C4a run sits at g = 0.16 on step 4 and <= 0.08 after
// (DESIGN §3), so nothing is gained above 1/2.
constexpr double kUpd32Tau = 0.5;
constexpr int kUpd32Log = 64;  // steps whose gate value is kept (rbl_upd32_gate_values)

// X -= l (l^T X) for every locked vector l in lock order (restarted.jl:1-21,
// restart_reorth_gpu!: one projection per locked vector, MGS over them).
int lock_reorth(rbl_ctx* ctx, double* X) {
  const int b = ctx->b;
  for (int j = 0; j < ctx->nlock; ++j) {
    const double* l = ctx->d_lock + (int64_t)j * ctx->nloc;
    CHK(gram(ctx, run1(l, 1), pan1(X, b), ctx->d_C, nullptr));
    CHK(tsmm_checked(ctx, run1(l, 1), ctx->d_C, b, pan1(X, b), -1.0, 1.0, nullptr));
  }
  return RBL_OK;
}

// RBL_OPT_CLOC_DERIVE applies to this run: options and plan state only, so every rank (and every
// run of a pair that differs in the SpMM's route alone) decides the same.  Block CGS and an
// all-resident basis are asked of both routes: the derivation through the partial reorth needs
// them, and with either unmet the run keeps the bits of the option-off routes.  On several ranks
// "all resident" must follow from the option (RBL_OPT_DEVICE_BLOCKS = 0): the automatic plan
// looks at each rank's own free memory, and the routes differ in their all-reduces.
bool cloc_derive_on(const rbl_ctx* ctx) {
  return ctx->cloc_derive && ctx->basis_bits == 64 && rowgram_ok(ctx->b) && (ctx->fuse & 3) == 3 &&
         ctx->reorth_order == 0 && !spilled(ctx) && (ctx->nranks == 1 || ctx->plan_all_resident);
}

// Reorth of the pair (Q_i, Q_{i-1}) = slots (i-1, i-2) of the fp64 basis:
//   flags bit 1: against the locked vectors, Q_{i-1} then Q_i (restarted.jl:54-55);
//   flags bit 0: against Q_1..Q_{i-2} (RBL_gpu.jl:59-81; block CGS, or the reference's
//                ascending-j block MGS with RBL_OPT_REORTH_ORDER = 1).
// i == 1 with bit 1: Q_1 against the locked vectors (restarted.jl:41).
int reorth_pair(rbl_ctx* ctx, int i, int flags) {
  const int b = ctx->b;
  double* Qi = slotp(ctx, i - 1);
  double* Qm = i >= 2 ? slotp(ctx, i - 2) : nullptr;
  // whatever route: only slots i - 1 and i - 2 are written (a step never has a valid shadow there;
  // rbl_reorth_last may be asked for an earlier pair)
  shadow_written(ctx, i - 2);
  if ((flags & 2) && ctx->nlock > 0) {
    StageScope t(ctx, RBL_STAGE_PART_REORTH);
    if (Qm) CHK(lock_reorth(ctx, Qm));
    CHK(lock_reorth(ctx, Qi));
  }
  if ((flags & 1) && i >= 3) {
    StageScope t(ctx, RBL_STAGE_PART_REORTH);
    const int nW = i - 2;
    const int nres = std::min(nW, ctx->resident);  // HBM-resident part of W
    // the last update of the pair also forms this step's local-reorth Gram Q_{i-1}^T Q_i
    // (RBL_OPT_FUSE bit 1; the update's 64-column fast path: b = 32)
    // (the same decision on every rank: the all-reduce below pairs up; a rank where the fast
    // path does not apply — too few rows, slab too small — forms its share with the Gram kernel)
    // RBL_OPT_CLOC_DERIVE: S_CLOC holds G = Q_{i-1}^T Q_i of the pair as it stands (formed with
    // Q_i, nothing touched the pair since), and block CGS is about to form C = W^T [Q_i | Q_{i-1}]
    // = [Ci | Cm] over all of W: afterwards Q'_{i-1}^T Q'_i = G - Cm^T Ci + Cm^T (W^T W - I) Ci,
    // the last term dropped (|Cm| |Ci| |W^T W - I|, far below the rounding of G).  The update
    // then runs plain: no cross-Gram epilogue, no partials, no all-reduce.
    const bool derive = cloc_derive_on(ctx) && b == 32 && ctx->cloc_step == i && !ctx->cloc_final &&
                        !((flags & 2) && ctx->nlock > 0) && nres == nW;
    const bool xg = (ctx->fuse & 2) && b == 32 && !derive;
    const int xg_parts = tsmm44_xg_grid(ctx->nloc);
    const bool xslab_ok = (size_t)(xg_parts + reduce_scratch_splits(xg_parts)) * b * b <= ctx->slab_elems;
    int xgrid = 0;
    auto update = [&](const PanelRun& W, bool last) -> int {
      const bool here = xg && last && xslab_ok;
      return tsmm_checked(ctx, W, ctx->d_C, 2 * b, pan2(Qi, Qm, b), -1.0, 1.0, nullptr,
                          here ? ctx->d_slab : nullptr, here ? &xgrid : nullptr);
    };
    if (ctx->reorth_order == 0) {  // block CGS: one Gram over every resident j, one update
      PanelRun W;
      W.base = slotp(ctx, 0);
      W.stride = ctx->slot;
      W.count = nres;
      W.w = b;
      CHK(gram(ctx, W, pan2(Qi, Qm, b), ctx->d_C, nullptr));
      // RBL_OPT_UPD32: where the update runs plain (b = 32, all of W resident, no locked vectors on
      // this step, no cross-Gram epilogue: the derive branch, or RBL_OPT_FUSE without bit 1) and
      // d_C is rounding residue, W C is formed on fp32 MFMA.  Both kernels are enqueued and the
      // gate's flags let one run: the gate reads all-reduced values only, so every rank takes the
      // same route, and the routes differ in no collective.  The guards are options and plan
      // state, as cloc_derive_on's.
      const Panels Yp = pan2(Qi, Qm, b);
      // (a rank without rows, or with too few for the fp32 kernel, still counts the step)
      const bool gate32 = ctx->upd32 != 0 && b == 32 && !xg && nres == nW && !((flags & 2) && ctx->nlock > 0);
      const bool u32 = gate32 && ctx->nloc > 0 && tsmm44x32_ok(ctx->nloc, W, Yp);
      if (gate32) {
        upd32_gate(ctx->d_C, nW * b, 2 * b, kUpd32Tau, ctx->upd32 == 2, ctx->d_upd32,
                   ctx->d_upd32_g + (i % kUpd32Log), ctx->stream);
        HIPC(hipGetLastError());
      }
      if (u32) {
        // RBL_OPT_UPD32_SHADOW: the panels below shadow_valid come from the fp32 shadow, the
        // others (two per even step of a run) are rounded as ever and enter it — also when the
        // gate refuses, which the host cannot know: the shadow is valid up to nW either way.
        // (rbl_reorth_last on a full basis has one panel more than the shadow has slots)
        if (ctx->d_shadow && ctx->shadow_opt && nW <= ctx->max_blocks - 2) {
          tsmm44x32_shadow(ctx->nloc, W, ctx->d_C, 2 * b, Yp, ctx->d_upd32, ctx->d_shadow,
                           ctx->shadow_valid, ctx->d_upd32 + 4, ctx->d_C16, ctx->stream);
          ctx->shadow_valid = nW;
        } else {
          tsmm44x32(ctx->nloc, W, ctx->d_C, 2 * b, Yp, ctx->d_upd32, ctx->d_C16, ctx->stream);
        }
        HIPC(hipGetLastError());
        CHK(tsmm_checked(ctx, W, ctx->d_C, 2 * b, Yp, -1.0, 1.0, ctx->d_upd32 + 1));
      } else {  // (also a rank whose rows do not fit the fp32 kernel: fp64 whatever the gate says)
        CHK(update(W, nres == nW));
      }
    } else {  // ascending-j block MGS, exactly the reference order
      for (int j = 0; j < nres; ++j) {
        const PanelRun W = run1(slotp(ctx, j), b);
        CHK(gram(ctx, W, pan2(Qi, Qm, b), ctx->d_C, nullptr));
        CHK(update(W, j == nW - 1));
      }
    }
    // spilled blocks (host, final): streamed back one at a time, ascending j, each applied
    // as soon as it lands — hybrid_part_reorth!'s `copyto!(Qgj, Q[j]); part_reorth_gpu!`
    // (RBL_gpu.jl:65-68)
    for (int j = nres; j < nW; ++j) {
      int st = 0;
      const double* Wj = block_dev(ctx, j, i, &st);
      if (st) return fail(ctx, st, "partial reorth: H2D of a spilled block failed");
      CHK(gram(ctx, run1(Wj, b), pan2(Qi, Qm, b), ctx->d_C, nullptr));
      CHK(update(run1(Wj, b), j == nW - 1));
    }
    if (xg) {  // the partials of the last update (its Gram slab was reduced before it)
      if (xgrid > 0) {
        reduce_slab_many(ctx->d_slab, xgrid, (int64_t)b * b, smallp(ctx, S_CLOC), ctx->stream);
      } else if (ctx->nloc > 0) {
        const int sp = gram_splits(ctx->nloc, 1, b, b);
        gram_partial(ctx->nloc, run1(Qm, b), pan1(Qi, b), ctx->d_slab, sp, nullptr, ctx->stream);
        reduce_slab(ctx->d_slab, sp, (int64_t)b * b, smallp(ctx, S_CLOC), nullptr, ctx->stream);
      } else {
        HIPC(hipMemsetAsync(smallp(ctx, S_CLOC), 0, (size_t)b * b * sizeof(double), ctx->stream));
      }
      HIPC(hipGetLastError());
      CHK(allreduce(ctx, smallp(ctx, S_CLOC), (size_t)b * b));
      ctx->cloc_step = i;
      ctx->cloc_final = true;
      ctx->cloc_src = 0;
    }
    if (derive) {  // d_C still holds [Ci | Cm], all-reduced by the Gram
      cloc_sub(smallp(ctx, S_CLOC), ctx->d_C, nW, b, ctx->stream);
      HIPC(hipGetLastError());
      ctx->cloc_final = true;
      ctx->cloc_src = 2;
    }
  }
  return RBL_OK;
}

// Y = [Q_1 .. Q_nblocks] S_dev (S_dev device row-major (nblocks*b) x kcols): one run over the
// HBM-resident blocks, then every other block (streamed from the host when spilled)
int combine_blocks(rbl_ctx* ctx, int nblocks, int kcols, const double* d_S, double* Y) {
  const int b = ctx->b;
  const int nres = std::min(nblocks, ctx->resident);
  PanelRun X;
  X.base = slotp(ctx, 0);
  X.stride = ctx->slot;
  X.count = nres;
  X.w = b;
  CHK(tsmm_checked(ctx, X, d_S, kcols, pan1(Y, kcols), 1.0, 0.0, nullptr));
  for (int j = nres; j < nblocks; ++j) {
    int st = 0;
    const double* Qj = block_dev(ctx, j, ctx->nblocks, &st);
    if (st) return fail(ctx, st, "Ritz: H2D of a spilled block failed");
    CHK(tsmm_checked(ctx, run1(Qj, b), d_S + (int64_t)j * b * kcols, kcols, pan1(Y, kcols), 1.0,
                     1.0, nullptr));
  }
  return RBL_OK;
}

// Y (n_local x kcols, row-major) = [Q_1 .. Q_nblocks] S with S host (nblocks*b) x kcols
// column-major — the Ritz combination of RBL.jl:61-71 / RBL_gpu.jl:106-132 (fp64 basis).
int basis_combine(rbl_ctx* ctx, int nblocks, int kcols, const double* S, double* Y) {
  const int b = ctx->b;
  const int64_t rows = (int64_t)nblocks * b;
  DevBuf<double> d_Scm, d_S;
  HIPC(d_Scm.alloc(rows * kcols));
  HIPC(d_S.alloc(rows * kcols));
  HIPC(hipMemcpyAsync(d_Scm, S, rows * kcols * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  colmajor_to_rowmajor(d_Scm, rows, kcols, d_S, ctx->stream);
  const int st = combine_blocks(ctx, nblocks, kcols, d_S, Y);
  HIPC(hipStreamSynchronize(ctx->stream));
  return st;
}

// Y = [Q_1 .. Q_nblocks] S_dev over the fp32 basis, widened on load, V and S fp64 (P3: fp64
// Ritz): one launch over the resident blocks when the fp32-input tsmm44 applies, else each
// block widened into a scratch block and accumulated; spilled blocks stream from the host
int combine_blocks32(rbl_ctx* ctx, int nblocks, int kcols, const double* d_S, double* Y) {
  const int b = ctx->b;
  if (ctx->nloc <= 0) return RBL_OK;
  const int nres = std::min(nblocks, ctx->resident);
  int j0 = 0;
  if (tsmm44_ok(b, kcols, kcols) && nres > 0) {
    PanelRun X;
    X.base32 = slotp32(ctx, 0);
    X.stride = ctx->slot;
    X.count = nres;
    X.w = b;
    tsmm44_f32x(ctx->nloc, X, d_S, kcols, pan1(Y, kcols), 1.0, 0.0, ctx->stream);
    HIPC(hipGetLastError());
    j0 = nres;
  }
  if (j0 < nblocks) CHK(ensure_qm64(ctx));
  for (int j = j0; j < nblocks; ++j) {
    int st = 0;
    const float* Qj = block_dev32(ctx, j, ctx->nblocks, &st);
    if (st) return fail(ctx, st, "Ritz: H2D of a spilled block failed");
    cvt_f32_to_f64(Qj, ctx->d_Qm64, ctx->nloc * b, ctx->stream);
    CHK(tsmm_checked(ctx, run1(ctx->d_Qm64, b), d_S + (int64_t)j * b * kcols, kcols, pan1(Y, kcols),
                     1.0, j == 0 ? 0.0 : 1.0, nullptr));
  }
  return RBL_OK;
}

// fp32 basis: Gram C = W^T [X0, X1] over all ranks (fp32 MFMA per split, fp64 sum), C fp64
// [nW*b][xcount*b] — the FLOAT `temp` of RBL_gpu.jl:33,39,87 (rounded to f32 where applied).
int gram32(rbl_ctx* ctx, const float* Wb, int nW, const float* X0, const float* X1, int xcount,
           double* C) {
  const int b = ctx->b;
  const int splits = gram32_splits(ctx->nloc);
  const int64_t len = (int64_t)nW * b * xcount * b;
  if ((size_t)splits * len > ctx->slab_elems)
    return fail(ctx, RBL_ERR_INVALID, "internal: Gram slab too small (fp32)");
  if (ctx->nloc > 0) {
    gram32_partial(ctx->nloc, Wb, ctx->slot, nW, b, X0, X1, xcount, ctx->d_slab, splits, ctx->stream);
    reduce_slab(ctx->d_slab, splits, len, C, nullptr, ctx->stream);
  } else {
    HIPC(hipMemsetAsync(C, 0, len * sizeof(double), ctx->stream));
  }
  HIPC(hipGetLastError());
  return allreduce(ctx, C, (size_t)len);
}
// fp32 basis: [Y0, Y1] -= X C (X: nX fp32 slots from Xb), RBL_gpu.jl:34,40,88 in FLOAT.
int upd32(rbl_ctx* ctx, const float* Xb, int nX, const double* C, int ldc, float* Y0, float* Y1,
          int ycount) {
  if (ctx->nloc <= 0) return RBL_OK;
  tsmm32(ctx->nloc, Xb, ctx->slot, nX, ctx->b, C, ldc, Y0, Y1, ycount, -1.f, 1.f, ctx->stream);
  HIPC(hipGetLastError());
  return RBL_OK;
}

// Fused row op in one of the CholQR forms (RowOpArgs: mode 1 Gram only, mode 2 two-stage
// apply, Z for a cross Gram).  G: the Gram (mode 1) over all ranks; Gx: Z^T Y over all ranks
// (reduced only when reduce_x).
int rowop_ex(rbl_ctx* ctx, RowOpArgs a, double* G, double* Gx, bool reduce_x, bool comm_x = true) {
  const int b = ctx->b;
  const int gmax = rowgram_grid(ctx->nloc, kRowgramMaxPerCu);
  if ((size_t)2 * gmax * b * b > ctx->slab_elems)
    return fail(ctx, RBL_ERR_INVALID, "internal: row-op slab too small");
  if (G) a.slab = ctx->d_slab;
  if (a.Z) a.slab2 = ctx->d_slab + (size_t)gmax * b * b;
  // the cross-Gram launches (pass 2, and pass 3 when it runs) share one grid: the reduce
  // after pass 3 does not know which of them wrote the partials last
  const int xgrid = rowgram_grid(ctx->nloc, 2);
  int grid = a.Z ? xgrid : 0;
  a.grid_out = &grid;
  if (ctx->nloc > 0) {
    if (!rowgram_ex(ctx->nloc, b, a, grid, ctx->stream))
      return fail(ctx, RBL_ERR_INVALID, "internal: unsupported fused row-op form");
  } else {  // no rows on this rank: zero partials (the all-reduces still run on every rank)
    grid = 1;
    if (G) HIPC(hipMemsetAsync(a.slab, 0, (size_t)b * b * sizeof(double), ctx->stream));
    if (a.Z)
      HIPC(hipMemsetAsync(a.slab2, 0, (size_t)xgrid * b * b * sizeof(double), ctx->stream));
  }
  HIPC(hipGetLastError());
  if (G) {
    reduce_slab(ctx->d_slab, grid, (int64_t)b * b, G, a.skip, ctx->stream);
    CHK(allreduce(ctx, G, (size_t)b * b));
  }
  if (Gx && reduce_x) {
    reduce_slab(ctx->d_slab + (size_t)gmax * b * b, xgrid, (int64_t)b * b, Gx, nullptr, ctx->stream);
    if (comm_x) CHK(allreduce(ctx, Gx, (size_t)b * b));
  }
  return RBL_OK;
}

// The 3-term update with both sums (RBL_OPT_CLOC_DERIVE): U' = U - Q_i A_i, S_G = U'^T U' and
// S_CLOC = M = Q_i^T U' from one pass over Q_i and U, one all-reduce of 2 b^2.  The grid is
// rowop's, so S_G has the bits of the pass without M.
int rowop_3term_cloc(rbl_ctx* ctx, const double* Qi, double* U) {
  const int b = ctx->b;
  const int grid = rowgram_grid(ctx->nloc);
  const size_t bb = (size_t)b * b;
  if (2 * grid * bb > ctx->slab_elems) return fail(ctx, RBL_ERR_INVALID, "internal: row-op slab too small");
  double* slab2 = ctx->d_slab + grid * bb;
  if (ctx->nloc > 0) {
    RowOpArgs a;
    a.X = Qi;
    a.C = smallp(ctx, S_AI);
    a.ldc = b;
    a.Y = U;
    a.alpha = -1.0;
    a.beta = 1.0;
    a.slab = ctx->d_slab;
    a.Z = Qi;
    a.slab2 = slab2;
    if (!rowgram_ex(ctx->nloc, b, a, grid, ctx->stream))
      return fail(ctx, RBL_ERR_INVALID, "internal: unsupported fused row-op form");
  } else {  // no rows on this rank: zero shares (the all-reduce still runs)
    HIPC(hipMemsetAsync(ctx->d_slab, 0, 2 * grid * bb * sizeof(double), ctx->stream));
  }
  reduce_slab(ctx->d_slab, grid, (int64_t)bb, smallp(ctx, S_G), nullptr, ctx->stream);
  reduce_slab(slab2, grid, (int64_t)bb, smallp(ctx, S_CLOC), nullptr, ctx->stream);
  HIPC(hipGetLastError());
  return allreduce(ctx, smallp(ctx, S_G), 2 * bb);
}

// RBL_OPT_CLOC_DERIVE: M's entries are sums over the same rows as the direct Gram's, so with e
// the direct Gram's error the derived Q_i^T Q_{i+1} = (Q_i^T U') R^-1 carries at most E e from M
// and as much again from the apply U' R^-1 (E of k_cloc_gate).  Up to E = 4 (8 e at the worst,
// the bound tests/test_cloc_derived_host.py holds every step to) the derived one is taken,
// beyond it — and after a shifted Cholesky — the direct one.  E is 1.1 .. 2.4 on a hash-window
// run once the planted eigenvalues have converged, 6 .. 93 in the three steps before.
constexpr double kClocGateTau = 4.0;

// Tall-skinny QR of U (n_local x b) into Qout; B = R (b x b, upper, row-major) in S_RTOT.
// Shifted CholQR2 (+ a third pass after a shifted first pass).  `g1_ready`: S_G already holds
// U^T U (the fused 3-term update computed it); each apply computes the next pass's Gram in the
// same pass over the rows when b allows (rowop).
// Qout32 (fp32 basis): the final Q goes to Qout32 rounded to fp32 (Qout then holds only a
// pass-2 intermediate when the shifted pass 3 runs).
// Zloc (fp64 basis, RBL_OPT_FUSE bit 1): also form Zloc^T Q into S_CLOC — the next step's
// local-reorth coefficient (Zloc = Q_i, Q = Q_{i+1}).
// cloc_m (RBL_OPT_CLOC_DERIVE, with Zloc): S_CLOC holds M = Zloc^T U over all ranks and leaves as
// Zloc^T Q = M R1^-1 R2^-1, so no pass reads Zloc — unless U is graded (k_cloc_gate, decided on
// the device from R1): then the last pass forms Zloc^T Q2 as without cloc_m.
int tsqr(rbl_ctx* ctx, const double* U, double* Qout, bool g1_ready = false, float* Qout32 = nullptr,
         const double* Zloc = nullptr, bool cloc_m = false) {
  StageScope t(ctx, RBL_STAGE_QR);
  ctx->flags_clean = false;  // the flags below start from zero only after a memset or k_stash
  const int b = ctx->b;
  int* need3 = ctx->d_flags;      // [need3, skip3]
  int* status = ctx->d_flags + 2; // [breakdown, shifted count]
  double* G = smallp(ctx, S_G);
  const int* skip3 = need3 + 1;
  const bool fused = rowgram_ok(b);
  // Qout = Qout R^-1: in place while one wave owns whole rows (tsmm: b <= 64), else through
  // the scratch block T
  auto apply_inplace = [&](const int* skip) -> int {
    if (b <= 64)
      return tsmm_checked(ctx, run1(Qout, b), smallp(ctx, S_RINV), b, pan1(Qout, b), 1.0, 0.0, skip);
    CHK(tsmm_checked(ctx, run1(Qout, b), smallp(ctx, S_RINV), b, pan1(ctx->d_T, b), 1.0, 0.0, skip));
    copy_small(ctx->d_T, Qout, ctx->nloc * b, ctx->stream, skip);
    return RBL_OK;
  };
  // pass 1 (shift decided on device); the 3-pass form keeps R1^-1 (S_RINV1) for its last pass
  const bool three = fused && (ctx->fuse & 1);
  if (!g1_ready) CHK(gram(ctx, run1(U, b), pan1(U, b), G, nullptr));
  chol_step(G, b, ctx->n, 0, smallp(ctx, S_R), smallp(ctx, three ? S_RINV1 : S_RINV), smallp(ctx, S_RTOT),
            need3, status, nullptr, ctx->stream, smallp(ctx, S_CHS0));
  if (three) {
    // 3 passes: G2 = Gram of Q1 = U R1^-1 without storing Q1; then Q = (U R1^-1) R2^-1 in
    // one pass (Q1 recomputed bit for bit) — the same bits as the 4-pass form below
    int* gate = ctx->d_flags + 4;  // [derived, direct]
    if (cloc_m)
      cloc_gate(smallp(ctx, S_R), smallp(ctx, S_RINV1), b, need3, kClocGateTau, gate, ctx->stream);
    RowOpArgs a1;
    a1.X = U;
    a1.C = smallp(ctx, S_RINV1);
    a1.ldc = b;
    a1.mode = 1;
    a1.tri = true;  // R^-1
    CHK(rowop_ex(ctx, a1, G, nullptr, false));
    chol_step(G, b, ctx->n, 1, smallp(ctx, S_R), smallp(ctx, S_RINV), smallp(ctx, S_RTOT), need3,
              status, nullptr, ctx->stream, smallp(ctx, S_CHS0));
    if (cloc_m) cloc_rinv2(smallp(ctx, S_CLOC), smallp(ctx, S_RINV1), smallp(ctx, S_RINV), b, ctx->stream);
    RowOpArgs a2;
    a2.X = U;
    a2.C = smallp(ctx, S_RINV1);
    a2.C2 = smallp(ctx, S_RINV);
    a2.ldc = b;
    a2.tri = true;  // R1^-1, R2^-1
    a2.Y = Qout;
    a2.Y32 = Qout32;
    a2.f64flag = Qout32 ? need3 : nullptr;
    a2.mode = 2;
    if (cloc_m) {
      // one of two launches runs (device gate): the plain pass where the derived coefficient
      // stands, the pass with the cross Gram Zloc^T Q2 (into S_CX) where U is too graded for it
      a2.skip = gate + 1;
      CHK(rowop_ex(ctx, a2, nullptr, nullptr, false));
      a2.skip = gate;
      a2.Z = Zloc;
      CHK(rowop_ex(ctx, a2, nullptr, smallp(ctx, S_CX), true, false));
    } else {
      a2.Z = Zloc;
      // Zloc: this rank's share of Zloc^T Q2 now, all-reduced below with the pass-3 Gram
      CHK(rowop_ex(ctx, a2, nullptr, Zloc ? smallp(ctx, S_CLOC) : nullptr, Zloc != nullptr, false));
    }
    // pass 3 only after a shifted first pass (device flag; kernels early-exit otherwise).  Its
    // Gram's all-reduce runs either way (the host does not know the flag) and carries Zloc^T Q2
    // in the same call (S_CLOC follows S_G; cloc_m: S_CX precedes it)
    CHK(gram(ctx, run1(Qout, b), pan1(Qout, b), G, skip3, Zloc == nullptr));
    if (cloc_m) {
      CHK(allreduce(ctx, smallp(ctx, S_CX), (size_t)2 * b * b));
      copy_small(smallp(ctx, S_CX), smallp(ctx, S_CLOC), (int64_t)b * b, ctx->stream, gate);
    } else if (Zloc) {
      CHK(allreduce(ctx, G, (size_t)2 * b * b));
    }
    chol_step(G, b, ctx->n, 1, smallp(ctx, S_R), smallp(ctx, S_RINV), smallp(ctx, S_RTOT), need3,
              status, skip3, ctx->stream, smallp(ctx, S_CHS0));
    RowOpArgs a3;
    a3.X = Qout;
    a3.C = smallp(ctx, S_RINV);
    a3.ldc = b;
    a3.tri = true;
    a3.Y = Qout;
    a3.skip = skip3;
    a3.Y32 = Qout32;
    a3.mode = 0;
    CHK(rowop_ex(ctx, a3, nullptr, nullptr, false));
    // after a third pass Q3 = Q2 R3^-1: Zloc^T Q3 = (Zloc^T Q2) R3^-1 (no-op unless it ran)
    if (Zloc) cloc_rinv(smallp(ctx, S_CLOC), smallp(ctx, S_RINV), b, skip3, ctx->stream);
    HIPC(hipGetLastError());
    return RBL_OK;
  }
  if (Zloc) return fail(ctx, RBL_ERR_INVALID, "internal: local-reorth Gram fusion needs the 3-pass QR");
  if (fused) {
    CHK(rowop(ctx, U, smallp(ctx, S_RINV), Qout, 1.0, 0.0, G, nullptr, nullptr, nullptr, nullptr, true));
  } else {
    CHK(tsmm_checked(ctx, run1(U, b), smallp(ctx, S_RINV), b, pan1(Qout, b), 1.0, 0.0, nullptr));
    CHK(gram(ctx, run1(Qout, b), pan1(Qout, b), G, nullptr));
  }
  // pass 2
  chol_step(G, b, ctx->n, 1, smallp(ctx, S_R), smallp(ctx, S_RINV), smallp(ctx, S_RTOT), need3,
            status, nullptr, ctx->stream, smallp(ctx, S_CHS0));
  if (fused) {  // in place; the Gram feeds pass 3 when a shifted first pass asked for it
    // (fp32 basis: the result goes straight to Qout32 unless pass 3 follows)
    CHK(rowop(ctx, Qout, smallp(ctx, S_RINV), Qout, 1.0, 0.0, G, nullptr, nullptr, Qout32,
              Qout32 ? need3 : nullptr, true));
  } else {
    CHK(apply_inplace(nullptr));
    CHK(gram(ctx, run1(Qout, b), pan1(Qout, b), G, skip3));
  }
  // pass 3 only after a shifted first pass (device flag; kernels early-exit otherwise)
  chol_step(G, b, ctx->n, 1, smallp(ctx, S_R), smallp(ctx, S_RINV), smallp(ctx, S_RTOT), need3,
            status, skip3, ctx->stream, smallp(ctx, S_CHS0));
  if (fused) {
    CHK(rowop(ctx, Qout, smallp(ctx, S_RINV), Qout, 1.0, 0.0, nullptr, skip3, nullptr, Qout32,
              nullptr, true));
  } else {
    CHK(apply_inplace(skip3));
    if (Qout32) cvt_f64_to_f32(Qout, Qout32, ctx->nloc * b, ctx->stream);
  }
  HIPC(hipGetLastError());
  return RBL_OK;
}

// Bring Q (n_local x b, local rows) into the halo-extended buffer for SpMM.  copy_local
// false: only the neighbours' rows land there (the band-tile SpMM reads the own rows from Q
// itself, CsrDev::qloc), saving a read + write of the whole local block per step.
int halo_exchange(rbl_ctx* ctx, const double* Q, const double** Qin, int64_t* off,
                  bool copy_local = true, hipStream_t st = nullptr) {
  if (ctx->nranks == 1) {
    *Qin = Q;
    *off = 0;
    return RBL_OK;
  }
  if (!st) st = ctx->stream;
  StageScope t(ctx, RBL_STAGE_COMM, st);
  const int b = ctx->b;
  CHK(ensure_qext(ctx, b, st));
  double* ext = ctx->d_qext;
  ctx->ghost_active = use_ghost(ctx, b);
  if (ctx->ghost_active) {  // indexed halo: pack the asked-for rows, receive into the ghost slots
    gather_rows(Q, ctx->d_send_idx, ctx->n_send, b, ctx->d_sendbuf, st);
    HIPC(hipGetLastError());
    std::vector<Comm::Xfer> x(ctx->nranks);
    for (int q = 0; q < ctx->nranks; ++q) {
      if (q == ctx->rank) continue;
      x[q].send = ctx->d_sendbuf + ctx->send_off[q] * b;
      x[q].nsend = (size_t)ctx->send_cnt[q] * b;
      x[q].recv = ext + ctx->ghost_off[q] * b;
      x[q].nrecv = (size_t)ctx->ghost_cnt[q] * b;
    }
    CHK(exchange(ctx, x, st));
    ctx->ghost_local = Q;
    *Qin = ext;
    *off = 0;
    return RBL_OK;
  }
  if (copy_local)
    HIPC(hipMemcpyAsync(ext + (ctx->r0 - ctx->ext_lo) * b, Q, ctx->nloc * b * sizeof(double),
                        hipMemcpyDeviceToDevice, st));
  std::vector<Comm::Xfer> x(ctx->nranks);
  for (int q = 0; q < ctx->nranks; ++q) {
    if (q == ctx->rank) continue;
    const int64_t gl = ctx->give_lo[q], gh = ctx->give_hi[q];
    if (gh > gl) {
      x[q].send = Q + (gl - ctx->r0) * b;
      x[q].nsend = (size_t)(gh - gl) * b;
    }
    const int64_t nl = ctx->need_lo[q], nh = ctx->need_hi[q];
    if (nh > nl) {
      x[q].recv = ext + (nl - ctx->ext_lo) * b;
      x[q].nrecv = (size_t)(nh - nl) * b;
    }
  }
  CHK(exchange(ctx, x, st));
  *Qin = ext;
  *off = ctx->ext_lo;
  return RBL_OK;
}

// fp32 halo exchange (the fp32 basis read directly by the band-tile SpMM): the same row
// ranges as halo_exchange, fp32 rows moved as byte-identical pairs (b is even)
int halo_exchange32(rbl_ctx* ctx, const float* Q, const float** Qin, int64_t* off,
                    bool copy_local = true) {
  if (ctx->nranks == 1) {
    *Qin = Q;
    *off = 0;
    return RBL_OK;
  }
  StageScope t(ctx, RBL_STAGE_COMM);
  const int b = ctx->b;
  float* ext = reinterpret_cast<float*>(ctx->d_qext.p);
  if (copy_local)
    HIPC(hipMemcpyAsync(ext + (ctx->r0 - ctx->ext_lo) * b, Q, ctx->nloc * b * sizeof(float),
                        hipMemcpyDeviceToDevice, ctx->stream));
  std::vector<Comm::Xfer> x(ctx->nranks);
  for (int q = 0; q < ctx->nranks; ++q) {
    if (q == ctx->rank) continue;
    const int64_t gl = ctx->give_lo[q], gh = ctx->give_hi[q];
    if (gh > gl) {
      x[q].send = reinterpret_cast<const double*>(Q + (gl - ctx->r0) * b);
      x[q].nsend = (size_t)(gh - gl) * b / 2;
    }
    const int64_t nl = ctx->need_lo[q], nh = ctx->need_hi[q];
    if (nh > nl) {
      x[q].recv = reinterpret_cast<double*>(ext + (nl - ctx->ext_lo) * b);
      x[q].nrecv = (size_t)(nh - nl) * b / 2;
    }
  }
  CHK(exchange(ctx, x, ctx->stream));
  *Qin = ext;
  *off = ctx->ext_lo;
  return RBL_OK;
}

// A/B switches of the variants build (tools/build_variant.sh with -DRBL_VARIANTS): the plain
// D2H copy instead of the staged one (RBL_D2H_DIRECT), the one-pass Ritz (RBL_RITZ_SERIAL)
#ifdef RBL_VARIANTS
bool d2h_direct() { return std::getenv("RBL_D2H_DIRECT") != nullptr; }
bool ritz_serial() { return std::getenv("RBL_RITZ_SERIAL") != nullptr; }
#else
constexpr bool d2h_direct() { return false; }
constexpr bool ritz_serial() { return false; }
#endif

// one step's record in the async stash: A_i, R_tot (b x b each) and 4 int flags (2 doubles)
size_t stash_rec(int b) { return (size_t)2 * b * b + 2; }

// the side stream of the host spill (D2H copies of finished blocks) and its events
int ensure_spill_stream(rbl_ctx* ctx) {
  if (ctx->cstream) return RBL_OK;
  HIPC(hipStreamCreateWithFlags(&ctx->cstream, hipStreamNonBlocking));
  HIPC(hipEventCreateWithFlags(&ctx->ev_fin, hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&ctx->ev_d2h[0], hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&ctx->ev_d2h[1], hipEventDisableTiming));
  return RBL_OK;
}
// The staged D2H of the Ritz vectors (d2h_staged): two pinned 64 MiB slots and their events,
// kept for the context's life.  Pinning them costs ~20-30 ms, so rbl_start allocates them with
// the run's buffers when a Ritz result will take the staged path (one basis block >= 256 MiB),
// instead of the first rbl_ritz of the context paying it (profiles/r05_ttk_probe.log).
constexpr size_t kD2HPiece = size_t(64) << 20;
int ensure_d2h_slots(rbl_ctx* ctx) {
  for (int s = 0; s < 2; ++s) {
    if (!ctx->h_d2h[s]) HIPC(ctx->h_d2h[s].alloc(kD2HPiece, hipHostMallocDefault));
    if (!ctx->ev_d2h_slot[s]) HIPC(hipEventCreateWithFlags(&ctx->ev_d2h_slot[s], hipEventDisableTiming));
  }
  return RBL_OK;
}

// The pipelined Ritz vectors' side stream and events (ritz_pipelined).  A stream's first launch
// costs ~25 ms (measured: the first pipelined rbl_ritz of a process took 60 ms against 31 ms for
// the next), so rbl_start creates them with the staging slots and runs one empty launch on the
// stream, instead of a time-to-k's Ritz step paying it.
int ensure_ritz_stream(rbl_ctx* ctx) {
  if (!ctx->rstream) {
    HIPC(hipStreamCreateWithFlags(&ctx->rstream, hipStreamNonBlocking));
    copy_small(ctx->d_small, ctx->d_small, 0, ctx->rstream);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->rstream));
  }
  for (hipEvent_t& e : ctx->ev_ritz)
    if (!e) HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return RBL_OK;
}

// ---- the pushed half of the split halo (prepare_push) ----
bool push_on(const rbl_ctx* ctx) { return ctx->push && ctx->ghost_active && ctx->nranks > 1; }

int ensure_push(rbl_ctx* ctx, int b) {
  const size_t need = (size_t)std::max<int64_t>(std::max(ctx->push_rows, ctx->n_send), 1) * b;
  if (ctx->d_pushbuf && ctx->push_cap >= need) return RBL_OK;
  HIPC(hipStreamSynchronize(ctx->stream));
  if (ctx->hstream) HIPC(hipStreamSynchronize(ctx->hstream));
  ctx->d_pushbuf.reset();
  ctx->d_precv.reset();
  ctx->push_cap = 0;
  HIPC(ctx->d_pushbuf.alloc(need));
  HIPC(ctx->d_precv.alloc(need));
  ctx->push_cap = need;
  return RBL_OK;
}

// partial rows for the peers' ghost slots from the own rows of Q (n_local x b)
int push_products(rbl_ctx* ctx, const double* Q, int b, hipStream_t st) {
  StageScope t(ctx, RBL_STAGE_AQ, st);
  CHK(ensure_push(ctx, b));
  const auto& P = ctx->push_tier;
  CsrDev::Tier T;
  T.rowptr = P.rowptr;
  T.col = P.col;
  T.val = P.val;
  T.ntasks = P.ntasks;
  T.nlong = P.nlong;
  T.trow = P.trow;
  T.tinfo = P.tinfo;
  T.slot_k0 = P.slot_k0;
  T.lrow = P.lrow;
  T.lslot = P.lslot;
  T.scratch = P.scratch;
  spmm_seg_tier(T, Q, ctx->r0, b, ctx->d_pushbuf, st);
  HIPC(hipGetLastError());
  return RBL_OK;
}

// partials out to the owners of the ghost slots, in from the peers for the rows they asked for
// (the reverse of halo_exchange's directions and counts)
int push_exchange(rbl_ctx* ctx, int b, hipStream_t st) {
  StageScope t(ctx, RBL_STAGE_COMM, st);
  std::vector<Comm::Xfer> x(ctx->nranks);
  for (int q = 0; q < ctx->nranks; ++q) {
    if (q == ctx->rank) continue;
    x[q].send = ctx->d_pushbuf + ctx->ghost_off[q] * b;
    x[q].nsend = (size_t)ctx->ghost_cnt[q] * b;
    x[q].recv = ctx->d_precv + ctx->send_off[q] * b;
    x[q].nrecv = (size_t)ctx->send_cnt[q] * b;
  }
  CHK(exchange(ctx, x, st));
  return RBL_OK;
}

int push_finish(rbl_ctx* ctx, double* U, int b, hipStream_t st) {
  StageScope t(ctx, RBL_STAGE_AQ, st);
  push_add(ctx->d_ps_rows, ctx->d_ps_ptr, ctx->d_ps_slot, ctx->n_ps_rows, ctx->d_precv, b, U, st);
  HIPC(hipGetLastError());
  return RBL_OK;
}

// the whole pushed half on one stream, after apply_A: products, exchange, add
int push_halo(rbl_ctx* ctx, const double* Q, int b, double* U) {
  if (!push_on(ctx)) return RBL_OK;
  CHK(push_products(ctx, Q, b, ctx->stream));
  CHK(push_exchange(ctx, b, ctx->stream));
  return push_finish(ctx, U, b, ctx->stream);
}

void free_run(rbl_ctx* ctx) {
  // the side streams first: the spill copies read the basis, the halo stream the push buffers
  if (ctx->cstream) hipStreamSynchronize(ctx->cstream);
  if (ctx->hstream) hipStreamSynchronize(ctx->hstream);
  static_cast<RunBufs&>(*ctx) = RunBufs{};
  ctx->resident = INT32_MAX;
  ctx->d2h_pending[0] = ctx->d2h_pending[1] = false;
  ctx->basis_bits = 64;
  ctx->qext_cap = 0;
  ctx->push_cap = 0;
  ctx->nlock = ctx->lock_cap = 0;
  ctx->arrow_W_cap = ctx->tr_S_cap = 0;
  ctx->arrow_kb = 0;
  ctx->filt_cols = 0;
  ctx->ritz_k = 0;
  ctx->dv_pin = ctx->dv_hist = nullptr;
  ctx->nblocks = 0;
  ctx->b = 0;
  ctx->have_bprev = false;
  ctx->shadow_valid = 0;
  ctx->shadow_slot = 0;
  ctx->shadow_bytes = 0;
}

// the rank-one shift of a rectangular B and the buffers of its reductions
void free_rect_shift(rbl_ctx* ctx) {
  static_cast<RectShiftBufs&>(*ctx) = RectShiftBufs{};
  ctx->rect_ts_cols = 0;
  ctx->rect_shift = false;
}

// the low-rank update and the buffers of its passes
void free_lowrank(rbl_ctx* ctx) {
  static_cast<LowrankBufs&>(*ctx) = LowrankBufs{};
  ctx->lr_cols = 0;
  ctx->lr_r = ctx->lr_rp = 0;
}

// the preconditioner of rbl_solve
void free_precond(rbl_ctx* ctx) {
  static_cast<PrecondBufs&>(*ctx) = PrecondBufs{};
  ctx->pc_r = ctx->pc_rp = 0;
}

void free_matrix(rbl_ctx* ctx) {
  // the parts that are also released alone reset their own scalars; then every matrix buffer
  free_panels(ctx);
  free_tiers(ctx);
  free_rect_shift(ctx);
  free_lowrank(ctx);
  free_precond(ctx);
  static_cast<MatrixBufs&>(*ctx) = MatrixBufs{};
  ctx->bt_ng = 0;
  ctx->seg_ntasks = ctx->seg_nlong = 0;
  ctx->rect_y_cols = 0;
  ctx->arrow_kb = 0;  // a pending arrow step belongs to the operator its basis was built with
  ctx->rect = false;
  ctx->rect_m = 0;
  ctx->kernop = false;
  ctx->kern_d = ctx->kern_d4 = ctx->kern_kind = ctx->kern_degree = 0;
  ctx->kern_gamma = ctx->kern_coef0 = ctx->kern_nugget = 0.0;
  ctx->qfull_cols = 0;
  ctx->dense = false;
  ctx->dense_panels = 0;
  ctx->n = ctx->nloc = ctx->nnz = 0;
  ctx->ntiles = ctx->tiles_per_wg = 0;
  ctx->window_ok16 = ctx->window_ok32 = false;
  ctx->band_ok16 = ctx->band_ok32 = false;
  ctx->csr_dropped = false;
  ctx->relabeled = false;
}

// Exchange halo needs among ranks and size the extended buffer.
int setup_halo(rbl_ctx* ctx) {
  const int P = ctx->nranks;
  ctx->give_lo.assign(P, 0);
  ctx->give_hi.assign(P, 0);
  ctx->ext_lo = ctx->r0;
  ctx->ext_hi = ctx->r1;
  if (P == 1) return RBL_OK;
  for (int q = 0; q < P; ++q) {
    if (q == ctx->rank || ctx->need_hi[q] <= ctx->need_lo[q]) continue;
    ctx->ext_lo = std::min(ctx->ext_lo, ctx->need_lo[q]);
    ctx->ext_hi = std::max(ctx->ext_hi, ctx->need_hi[q]);
  }
  // all-gather the (lo,hi) need tables: row p of the table = what rank p needs from each q
  std::vector<int64_t> mine(2 * P);
  for (int q = 0; q < P; ++q) {
    mine[2 * q] = ctx->need_lo[q];
    mine[2 * q + 1] = ctx->need_hi[q];
  }
  std::vector<int64_t> all(2 * P * P);
  COMMC(ctx->comm->allgather_host(mine.data(), all.data(), 2 * P, ctx->stream, &ctx->err));
  for (int p = 0; p < P; ++p) {
    if (p == ctx->rank) continue;
    ctx->give_lo[p] = all[(size_t)p * 2 * P + 2 * ctx->rank];
    ctx->give_hi[p] = all[(size_t)p * 2 * P + 2 * ctx->rank + 1];
  }
  return RBL_OK;
}

// The CSR arrays of m rows and nnz nonzeros, the kCsrPad entries past the last zeroed.
int alloc_csr(rbl_ctx* ctx, int64_t m, int64_t nnz) {
  HIPC(ctx->d_rowptr.alloc(m + 1));
  HIPC(ctx->d_col.alloc(nnz + kCsrPad));
  HIPC(ctx->d_val.alloc(nnz + kCsrPad));
  HIPC(hipMemset(ctx->d_col + nnz, 0, kCsrPad * sizeof(int32_t)));
  HIPC(hipMemset(ctx->d_val + nnz, 0, kCsrPad * sizeof(double)));
  return RBL_OK;
}

// A generator's planted eigenvalues on the device (none: d_plant stays null).
int upload_plant(rbl_ctx* ctx, int nplant, const double* plant, DevBuf<double>& d_plant) {
  if (nplant <= 0) return RBL_OK;
  HIPC(d_plant.alloc(nplant));
  HIPC(hipMemcpy(d_plant, plant, nplant * sizeof(double), hipMemcpyHostToDevice));
  return RBL_OK;
}

// A generator's per-row counts (device, m int32) as the row pointer rp; sets ctx->nnz.
int counts_to_rowptr(rbl_ctx* ctx, const int32_t* d_cnt, int64_t m, std::vector<int64_t>& rp) {
  std::vector<int32_t> cnt(m);
  HIPC(hipMemcpyAsync(cnt.data(), d_cnt, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  rp.assign(m + 1, 0);
  for (int64_t i = 0; i < m; ++i) rp[i + 1] = rp[i] + cnt[i];
  ctx->nnz = rp[m];
  return RBL_OK;
}

// Upload a local CSR (0-based rowptr relative to the slice, global 0-based int64 columns).
int upload_csr(rbl_ctx* ctx, int64_t n, int64_t r0, int64_t r1, const int64_t* rowptr,
               const int64_t* colind, const double* val, int64_t base_ptr, int64_t base_idx) {
  free_run(ctx);
  free_matrix(ctx);
  const int64_t m = r1 - r0;
  const int64_t nnz = rowptr[m] - rowptr[0];
  std::vector<int64_t> rp(m + 1);
  for (int64_t i = 0; i <= m; ++i) rp[i] = rowptr[i] - rowptr[0];
  std::vector<int32_t> ci(nnz);
  const int64_t e0 = rowptr[0] - base_ptr;
  for (int64_t e = 0; e < nnz; ++e) {
    const int64_t c = colind[e0 + e] - base_idx;
    if (c < 0 || c >= n) return fail(ctx, RBL_ERR_INVALID, "column index out of range");
    if (c > INT32_MAX) return fail(ctx, RBL_ERR_INVALID, "n exceeds int32 column ids");
    ci[e] = (int32_t)c;
  }
  // rows must be column-sorted (SparseArrays guarantees it; the window kernel relies on it)
  for (int64_t i = 0; i < m; ++i)
    for (int64_t e = rp[i] + 1; e < rp[i + 1]; ++e)
      if (ci[e] < ci[e - 1]) return fail(ctx, RBL_ERR_INVALID, "row indices not sorted");
  ctx->n = n;
  ctx->r0 = r0;
  ctx->r1 = r1;
  ctx->nloc = m;
  ctx->nnz = nnz;
  CHK(alloc_csr(ctx, m, nnz));
  HIPC(hipMemcpy(ctx->d_rowptr, rp.data(), (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (nnz) {
    HIPC(hipMemcpy(ctx->d_col, ci.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(ctx->d_val, val + e0, nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  // halo needs: column footprint per owning rank
  const int P = ctx->nranks;
  ctx->need_lo.assign(P, 0);
  ctx->need_hi.assign(P, 0);
  if (P > 1) {
    std::vector<int64_t> lo(P), hi(P);
    for (int q = 0; q < P; ++q) { lo[q] = INT64_MAX; hi[q] = -1; }
    for (int64_t e = 0; e < nnz; ++e) {
      const int64_t c = ci[e];
      const int q = (int)(std::upper_bound(ctx->bounds.begin(), ctx->bounds.end(), c) -
                          ctx->bounds.begin()) - 1;
      lo[q] = std::min(lo[q], c);
      hi[q] = std::max(hi[q], c + 1);
    }
    for (int q = 0; q < P; ++q) {
      ctx->need_lo[q] = hi[q] < 0 ? 0 : lo[q];
      ctx->need_hi[q] = hi[q] < 0 ? 0 : hi[q];
    }
  }
  CHK(prepare_window(ctx, rp));
  return setup_halo(ctx);
}

// The halo of an unbanded local CSR (R-MAT, circuit): for every other rank q, the contiguous
// range of q's rows the local columns reference (col_footprint on the device).
int halo_from_footprint(rbl_ctx* ctx) {
  const int P = ctx->nranks;
  const int64_t nnz = ctx->nnz;
  ctx->need_lo.assign(P, 0);
  ctx->need_hi.assign(P, 0);
  if (P > 1 && nnz > 0) {
    DevBuf<int64_t> d_b;
    DevBuf<unsigned long long> d_lh;
    HIPC(d_b.alloc(P + 1));
    HIPC(d_lh.alloc(2 * P));
    std::vector<unsigned long long> lh(2 * P);
    for (int q = 0; q < P; ++q) { lh[q] = ~0ull; lh[P + q] = 0ull; }
    HIPC(hipMemcpy(d_b, ctx->bounds.data(), (P + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_lh, lh.data(), 2 * P * sizeof(unsigned long long), hipMemcpyHostToDevice));
    col_footprint(ctx->d_col, nnz, d_b, P, d_lh, d_lh + P, ctx->stream);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(lh.data(), d_lh, 2 * P * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < P; ++q) {
      if (q == ctx->rank || lh[P + q] == 0ull) continue;
      ctx->need_lo[q] = (int64_t)lh[q];
      ctx->need_hi[q] = (int64_t)lh[P + q];
    }
  }
  return RBL_OK;
}

}  // namespace

// =========================================================================================
extern "C" {

int rbl_abi_version(void) { return RBL_ABI_VERSION; }
int rbl_build_flags(void) {
#ifdef RBL_VARIANTS
  return RBL_BUILD_VARIANTS;
#else
  return 0;
#endif
}

int rbl_create(rbl_ctx** out, int device) {
  if (!out) return RBL_ERR_INVALID;
  rbl_ctx* ctx = new rbl_ctx();
  ctx->device = device;
  *out = ctx;
  HIPC(hipSetDevice(device));
  HIPC(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  ctx->bounds = {0, 0};
  return RBL_OK;
}

int rbl_get_unique_id(uint8_t unique_id[128]) {
  if (!unique_id) return RBL_ERR_INVALID;
  return rccl_unique_id(unique_id) == 0 ? RBL_OK : RBL_ERR_RCCL;
}

int rbl_comm_selftest(int device, char* msg, int msg_len) {
  // one-rank RCCL communicator through the production transport (RcclComm): the three
  // collective shapes on real device buffers, checked on the host
  std::string err;
  auto say = [&](const std::string& m) {
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", m.c_str());
  };
  if (hipSetDevice(device) != hipSuccess) { say("hipSetDevice failed"); return RBL_ERR_HIP; }
  uint8_t id[128];
  if (rccl_unique_id(id) != 0) { say("ncclGetUniqueId failed"); return RBL_ERR_RCCL; }
  Comm* c = make_rccl_comm(1, 0, id, &err);
  if (!c) { say("ncclCommInitRank: " + err); return RBL_ERR_RCCL; }
  hipStream_t st = nullptr;
  DevBuf<double> d;
  int rc = RBL_OK;
  const size_t n = 4096;
  std::vector<double> h(n), back(n);
  for (size_t k = 0; k < n; ++k) h[k] = 0.5 * (double)k - 7.0;
  if (hipStreamCreate(&st) != hipSuccess || d.alloc(2 * n) != hipSuccess ||
      hipMemcpy(d, h.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    say("HIP setup failed");
    rc = RBL_ERR_HIP;
  }
  if (rc == RBL_OK && c->allreduce_sum(d, n, st, &err) != 0) { say("allreduce: " + err); rc = RBL_ERR_RCCL; }
  if (rc == RBL_OK) {
    hipMemcpyAsync(back.data(), d, n * sizeof(double), hipMemcpyDeviceToHost, st);
    hipStreamSynchronize(st);
    if (back != h) { say("allreduce over one rank changed the data"); rc = RBL_ERR_RCCL; }
  }
  int64_t mine[3] = {11, -2, 1LL << 40}, all[3] = {0, 0, 0};
  if (rc == RBL_OK && c->allgather_host(mine, all, 3, st, &err) != 0) { say("allgather: " + err); rc = RBL_ERR_RCCL; }
  if (rc == RBL_OK && (all[0] != mine[0] || all[1] != mine[1] || all[2] != mine[2])) {
    say("allgather returned other values");
    rc = RBL_ERR_RCCL;
  }
  std::vector<Comm::Xfer> x(1);  // no peers: an empty grouped exchange
  if (rc == RBL_OK && c->exchange(x, st, &err) != 0) { say("exchange: " + err); rc = RBL_ERR_RCCL; }
  if (rc == RBL_OK && hipStreamSynchronize(st) != hipSuccess) { say("stream sync failed"); rc = RBL_ERR_HIP; }
  if (rc == RBL_OK) say(std::string("ok: ") + c->name());
  delete c;
  d.reset();
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

int rbl_create_dist(rbl_ctx** out, int device, int nranks, int rank, const uint8_t unique_id[128]) {
  if (!out || nranks < 1 || rank < 0 || rank >= nranks) return RBL_ERR_INVALID;
  int s = rbl_create(out, device);
  if (s != RBL_OK) return s;
  rbl_ctx* ctx = *out;
  ctx->nranks = nranks;
  ctx->rank = rank;
  if (nranks > 1) {
    if (!unique_id) return fail(ctx, RBL_ERR_INVALID, "rbl_create_dist: null unique_id");
    ctx->comm = make_rccl_comm(nranks, rank, unique_id, &ctx->err);
    if (!ctx->comm) return RBL_ERR_RCCL;
  }
  return RBL_OK;
}

int rbl_local_group_create(rbl_group** group, int nranks) {
  if (!group || nranks < 1) return RBL_ERR_INVALID;
  *group = reinterpret_cast<rbl_group*>(local_group_create(nranks));
  return RBL_OK;
}

int rbl_local_group_free(rbl_group* group) {
  local_group_release(reinterpret_cast<LocalGroup*>(group));
  return RBL_OK;
}

int rbl_create_local(rbl_ctx** out, int device, rbl_group* group, int rank) {
  if (!out || !group) return RBL_ERR_INVALID;
  int s = rbl_create(out, device);
  if (s != RBL_OK) return s;
  rbl_ctx* ctx = *out;
  ctx->comm = make_local_comm(reinterpret_cast<LocalGroup*>(group), rank, &ctx->err);
  if (!ctx->comm) return RBL_ERR_INVALID;
  ctx->nranks = ctx->comm->nranks;
  ctx->rank = rank;
  return RBL_OK;
}

int rbl_create_shm(rbl_ctx** out, int device, int nranks, int rank, const char* path) {
  if (!out || nranks < 1 || rank < 0 || rank >= nranks || !path) return RBL_ERR_INVALID;
  int s = rbl_create(out, device);
  if (s != RBL_OK) return s;
  rbl_ctx* ctx = *out;
  ctx->nranks = nranks;
  ctx->rank = rank;
  if (nranks > 1) {
    ctx->comm = make_shm_comm(nranks, rank, path, &ctx->err);
    if (!ctx->comm) return RBL_ERR_RCCL;
  }
  return RBL_OK;
}

int rbl_free(rbl_ctx* ctx) {
  if (!ctx) return RBL_OK;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  if (ctx->hstream) hipStreamSynchronize(ctx->hstream);
  free_run(ctx);
  free_matrix(ctx);
  for (auto e : ctx->ev_pool) hipEventDestroy(e);
  for (auto e : ctx->step_ev)
    if (e) hipEventDestroy(e);
  delete ctx->comm;
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  if (ctx->cstream) hipStreamDestroy(ctx->cstream);
  if (ctx->hstream) hipStreamDestroy(ctx->hstream);
  if (ctx->rstream) hipStreamDestroy(ctx->rstream);
  for (hipEvent_t e : ctx->ev_ritz)
    if (e) hipEventDestroy(e);
  if (ctx->ev_push_ready) hipEventDestroy(ctx->ev_push_ready);
  if (ctx->ev_push_done) hipEventDestroy(ctx->ev_push_done);
  for (hipEvent_t e : {ctx->ev_fin, ctx->ev_d2h[0], ctx->ev_d2h[1], ctx->ev_d2h_slot[0],
                       ctx->ev_d2h_slot[1], ctx->ev_qready, ctx->ev_halo})
    if (e) hipEventDestroy(e);
  static_cast<CtxBufs&>(*ctx) = CtxBufs{};
  delete ctx;
  return RBL_OK;
}

const char* rbl_last_error(const rbl_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rbl_device_memory(rbl_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes) {
  if (!ctx || !free_bytes || !total_bytes) return RBL_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  size_t fr = 0, tot = 0;
  HIPC(hipMemGetInfo(&fr, &tot));
  *free_bytes = (int64_t)fr;
  *total_bytes = (int64_t)tot;
  return RBL_OK;
}

int rbl_comm_info(rbl_ctx* ctx, int* nranks, int* rank, char* transport, int transport_len) {
  if (!ctx || !nranks || !rank) return RBL_ERR_INVALID;
  int cnt = 1;
  const char* name = "none";
  if (ctx->comm) {
    hipSetDevice(ctx->device);
    const int s = ctx->comm->count(&cnt, &ctx->err);
    if (s < 0) return s;
    name = ctx->comm->name();
  }
  *nranks = cnt;
  *rank = ctx->rank;
  if (transport && transport_len > 0) snprintf(transport, (size_t)transport_len, "%s", name);
  return RBL_OK;
}

int rbl_rccl_version(int* version, char* path, int path_len) {
  if (!version) return RBL_ERR_INVALID;
  std::string p, err;
  const int s = rbl::rccl_library(version, &p, &err);
  if (path && path_len > 0) snprintf(path, (size_t)path_len, "%s", s ? err.c_str() : p.c_str());
  return s ? RBL_ERR_RCCL : RBL_OK;
}

int rbl_set_option(rbl_ctx* ctx, int option, int64_t value) {
  if (!ctx) return RBL_ERR_INVALID;
  switch (option) {
    case RBL_OPT_TIMERS:
      if (value < 0 || value > 2) return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_TIMERS: 0, 1 or 2");
      ctx->timers = (int)value;
      return RBL_OK;
    case RBL_OPT_REORTH_ORDER:
      if (value < 0 || value > 1) return fail(ctx, RBL_ERR_INVALID, "reorth order must be 0|1");
      ctx->reorth_order = (int)value;
      return RBL_OK;
    case RBL_OPT_DEVICE_BLOCKS:
      if (value < -1 || value == 1 || value == 2 || value > INT32_MAX)
        return fail(ctx, RBL_ERR_INVALID, "device blocks: 0 (all), -1 (auto) or >= 3");
      ctx->dev_blocks_opt = (int)value;
      return RBL_OK;
    case RBL_OPT_SPMM_KERNEL:
      // option values are the kernel ids rbl_spmm_kernel_for reports (4, the dense panel GEMM,
      // follows from rbl_set_matrix_dense and is not selectable); internally the band tiles
      // are variant 4 and the segmented gather variant 5 (spmm.hip)
      if (value < 0 || value > 7 || value == 4)
        return fail(ctx, RBL_ERR_INVALID, "spmm kernel must be 0 (auto) or a kernel id 1, 2, 3, 5, 6, 7");
      ctx->spmm_variant = value == 5 ? 4 : value == 6 ? 5 : (int)value;
      return RBL_OK;
    case RBL_OPT_SPLIT_HALO: ctx->split_halo = value != 0; return RBL_OK;
    case RBL_OPT_HALO_OVERLAP: ctx->halo_overlap = value != 0; return RBL_OK;
    case RBL_OPT_HALO_PUSH:
      if (value < 0 || value > 2) return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_HALO_PUSH must be 0|1|2");
      ctx->halo_push_opt = (int)value;
      return RBL_OK;
    case RBL_OPT_KEEP_CSR: ctx->keep_csr = value != 0; return RBL_OK;
    case RBL_OPT_RELABEL:
      if (value < 0 || value > 1) return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_RELABEL must be 0|1");
      ctx->relabel_opt = (int)value;
      return RBL_OK;
    case RBL_OPT_FUSE:
      if (value < 0 || value > 7) return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_FUSE is a 3-bit mask");
      ctx->fuse = (int)value;
      return RBL_OK;
    case RBL_OPT_CLOC_DERIVE:
      if (value < 0 || value > 1) return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_CLOC_DERIVE must be 0|1");
      ctx->cloc_derive = value != 0;
      return RBL_OK;
    case RBL_OPT_UPD32:
      if (value < 0 || value > 2) return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_UPD32 must be 0|1|2");
      ctx->upd32 = (int)value;
      return RBL_OK;
    case RBL_OPT_UPD32_SHADOW:
      if (value < 0 || value > 1) return fail(ctx, RBL_ERR_INVALID, "RBL_OPT_UPD32_SHADOW must be 0|1");
      ctx->shadow_opt = (int)value;
      return RBL_OK;
    default: return fail(ctx, RBL_ERR_INVALID, "unknown option");
  }
}

int rbl_set_matrix_csc(rbl_ctx* ctx, int64_t n, int64_t nnz, const int64_t* colptr,
                       const int64_t* rowval, const double* nzval, int index_base) {
  if (!ctx || n < 1 || nnz < 0 || !colptr || (nnz && (!rowval || !nzval)) ||
      (index_base != 0 && index_base != 1))
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_csc: bad arguments");
  if (colptr[n] - colptr[0] != nnz) return fail(ctx, RBL_ERR_INVALID, "colptr[n] != nnz");
  HIPC(hipSetDevice(ctx->device));
  // symmetric: column slice [r0,r1) of CSC == row slice of CSR
  std::vector<int64_t> rp(n + 1);
  for (int64_t i = 0; i <= n; ++i) rp[i] = colptr[i] - colptr[0];
  ctx->bounds.assign(ctx->nranks + 1, 0);
  rbl_plan_row_partition(n, rp.data(), ctx->nranks, ctx->bounds.data());
  const int64_t r0 = ctx->bounds[ctx->rank], r1 = ctx->bounds[ctx->rank + 1];
  return upload_csr(ctx, n, r0, r1, colptr + r0, rowval, nzval, index_base, index_base);
}

int rbl_set_matrix_csr_rows(rbl_ctx* ctx, int64_t n, int64_t row_begin, int64_t row_end,
                            const int64_t* rowptr, const int64_t* colind, const double* val,
                            int index_base) {
  if (!ctx || n < 1 || row_begin < 0 || row_end < row_begin || row_end > n || !rowptr ||
      (index_base != 0 && index_base != 1))
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_csr_rows: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  // the partition is the callers' (every rank's [row_begin,row_end) must tile [0,n))
  if (ctx->nranks > 1) {
    int64_t mine[2] = {row_begin, row_end};
    std::vector<int64_t> all(2 * ctx->nranks);
    COMMC(ctx->comm->allgather_host(mine, all.data(), 2, ctx->stream, &ctx->err));
    ctx->bounds.assign(ctx->nranks + 1, 0);
    for (int p = 0; p < ctx->nranks; ++p) {
      if (all[2 * p] != (p == 0 ? 0 : all[2 * p - 1]))
        return fail(ctx, RBL_ERR_INVALID, "row slices must tile [0,n) in rank order");
      ctx->bounds[p + 1] = all[2 * p + 1];
    }
    if (ctx->bounds[ctx->nranks] != n) return fail(ctx, RBL_ERR_INVALID, "row slices != n");
  } else {
    if (row_begin != 0 || row_end != n)
      return fail(ctx, RBL_ERR_INVALID, "single rank must own all rows");
    ctx->bounds = {0, n};
  }
  return upload_csr(ctx, n, row_begin, row_end, rowptr, colind, val, index_base, index_base);
}

int rbl_set_matrix_dense(rbl_ctx* ctx, int64_t n, int64_t row_begin, int64_t row_end,
                         const double* A, int64_t lda) {
  if (!ctx || n < 1 || row_begin < 0 || row_end < row_begin || row_end > n || !A ||
      lda < row_end - row_begin || lda < 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_dense: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  free_run(ctx);
  free_matrix(ctx);
  ctx->bounds.assign(ctx->nranks + 1, 0);
  if (ctx->nranks > 1) {  // the row slices must tile [0, n) in rank order
    int64_t mine[2] = {row_begin, row_end};
    std::vector<int64_t> all(2 * ctx->nranks);
    COMMC(ctx->comm->allgather_host(mine, all.data(), 2, ctx->stream, &ctx->err));
    for (int p = 0; p < ctx->nranks; ++p) {
      if (all[2 * p] != (p == 0 ? 0 : all[2 * p - 1]))
        return fail(ctx, RBL_ERR_INVALID, "row slices must tile [0,n) in rank order");
      ctx->bounds[p + 1] = all[2 * p + 1];
    }
    if (ctx->bounds[ctx->nranks] != n) return fail(ctx, RBL_ERR_INVALID, "row slices != n");
  } else {
    if (row_begin != 0 || row_end != n) return fail(ctx, RBL_ERR_INVALID, "one rank holds all rows");
    ctx->bounds[1] = n;
  }
  const int64_t m = row_end - row_begin;
  ctx->n = n;
  ctx->r0 = row_begin;
  ctx->r1 = row_end;
  ctx->nloc = m;
  ctx->nnz = m * n;
  ctx->dense = true;
  ctx->dense_panels = (n + 31) / 32;
  const int64_t P = ctx->dense_panels;
  const int64_t ml = std::max<int64_t>(m, 1);
  HIPC(ctx->d_dense.alloc((size_t)P * ml * 32));
  HIPC(ctx->d_qfull.alloc((size_t)P * 32 * 64));
  HIPC(hipMemsetAsync(ctx->d_qfull, 0, (size_t)P * 32 * 64 * sizeof(double), ctx->stream));
  ctx->qfull_cols = 64;
  // column-major slice -> row-major 32-column panels, one panel at a time through a scratch
  DevBuf<double> d_tmp;
  HIPC(d_tmp.alloc((size_t)ml * 32));
  for (int64_t p = 0; p < P && m > 0; ++p) {
    const int64_t c0 = 32 * p, nc = std::min<int64_t>(32, n - c0);
    if (nc < 32) HIPC(hipMemsetAsync(d_tmp, 0, (size_t)m * 32 * sizeof(double), ctx->stream));
    HIPC(hipMemcpy2DAsync(d_tmp, m * sizeof(double), A + c0 * lda, lda * sizeof(double),
                          m * sizeof(double), nc, hipMemcpyHostToDevice, ctx->stream));
    colmajor_to_rowmajor(d_tmp, m, 32, ctx->d_dense + p * m * 32, ctx->stream);
  }
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  d_tmp.reset();
  // every rank needs all n rows of Q
  const int Pr = ctx->nranks;
  ctx->need_lo.assign(Pr, 0);
  ctx->need_hi.assign(Pr, 0);
  for (int q = 0; q < Pr; ++q) {
    ctx->need_lo[q] = ctx->bounds[q];
    ctx->need_hi[q] = ctx->bounds[q + 1];
  }
  return setup_halo(ctx);
}

int rbl_gen_matrix_hashwindow(rbl_ctx* ctx, int64_t n, int64_t halfwidth, double density,
                              uint64_t seed, int nplant, const double* plant) {
  if (!ctx || n < 1 || halfwidth < 0 || nplant < 0 || (nplant > 0 && !plant) || n > INT32_MAX)
    return fail(ctx, RBL_ERR_INVALID, "rbl_gen_matrix_hashwindow: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  free_run(ctx);
  free_matrix(ctx);
  const int P = ctx->nranks;
  ctx->bounds.assign(P + 1, 0);
  for (int p = 0; p <= P; ++p) ctx->bounds[p] = n * p / P;  // uniform rows: ~uniform nnz
  const int64_t r0 = ctx->bounds[ctx->rank], r1 = ctx->bounds[ctx->rank + 1], m = r1 - r0;
  ctx->n = n;
  ctx->r0 = r0;
  ctx->r1 = r1;
  ctx->nloc = m;
  DevBuf<int32_t> d_cnt;
  HIPC(d_cnt.alloc(std::max<int64_t>(m, 1)));
  hw_count(n, halfwidth, density, seed, r0, r1, d_cnt, ctx->stream);
  std::vector<int64_t> rp;
  CHK(counts_to_rowptr(ctx, d_cnt, m, rp));
  d_cnt.reset();  // m counts, before the CSR
  CHK(alloc_csr(ctx, m, ctx->nnz));
  HIPC(hipMemcpy(ctx->d_rowptr, rp.data(), (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  DevBuf<double> d_plant;
  CHK(upload_plant(ctx, nplant, plant, d_plant));
  hw_fill(n, halfwidth, density, seed, r0, r1, ctx->d_rowptr, nplant, d_plant, ctx->d_col,
          ctx->d_val, ctx->stream);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  d_plant.reset();  // before the formats are built, so their allocations are placed as ever
  ctx->need_lo.assign(P, 0);
  ctx->need_hi.assign(P, 0);
  for (int q = 0; q < P; ++q) {  // analytic footprint of the window
    const int64_t lo = std::max(ctx->bounds[q], std::max<int64_t>(0, r0 - halfwidth));
    const int64_t hi = std::min(ctx->bounds[q + 1], std::min<int64_t>(n, r1 + halfwidth));
    if (hi > lo && q != ctx->rank) {
      ctx->need_lo[q] = lo;
      ctx->need_hi[q] = hi;
    }
  }
  CHK(prepare_window(ctx, rp));
  return setup_halo(ctx);
}

int rbl_gen_matrix_circuit(rbl_ctx* ctx, int64_t n, int64_t width, double p_edge, uint64_t seed,
                           int nplant, const double* plant) {
  if (!ctx || n < 1 || width < 1 || nplant < 0 || (nplant > 0 && !plant) || n > INT32_MAX ||
      !(p_edge >= 0.0 && p_edge <= 1.0))
    return fail(ctx, RBL_ERR_INVALID, "rbl_gen_matrix_circuit: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  free_run(ctx);
  free_matrix(ctx);
  const int P = ctx->nranks;
  ctx->bounds.assign(P + 1, 0);
  for (int q = 0; q <= P; ++q) ctx->bounds[q] = n * q / P;  // <= 5 nonzeros per row: uniform
  const int64_t r0 = ctx->bounds[ctx->rank], r1 = ctx->bounds[ctx->rank + 1], m = r1 - r0;
  ctx->n = n;
  ctx->r0 = r0;
  ctx->r1 = r1;
  ctx->nloc = m;
  DevBuf<int32_t> d_cnt;
  HIPC(d_cnt.alloc(std::max<int64_t>(m, 1)));
  circ_count(n, width, p_edge, seed, r0, r1, d_cnt, ctx->stream);
  HIPC(hipGetLastError());
  std::vector<int64_t> rp;
  CHK(counts_to_rowptr(ctx, d_cnt, m, rp));
  d_cnt.reset();  // m counts, before the CSR
  CHK(alloc_csr(ctx, m, ctx->nnz));
  HIPC(hipMemcpy(ctx->d_rowptr, rp.data(), (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  DevBuf<double> d_plant;
  CHK(upload_plant(ctx, nplant, plant, d_plant));
  circ_fill(n, width, p_edge, seed, r0, r1, ctx->d_rowptr, nplant, d_plant, ctx->d_col,
            ctx->d_val, ctx->stream);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  d_plant.reset();  // before the formats are built, so their allocations are placed as ever
  CHK(halo_from_footprint(ctx));
  CHK(prepare_window(ctx, rp));
  return setup_halo(ctx);
}

int rbl_gen_matrix_rmat(rbl_ctx* ctx, int64_t n, int scale, int64_t edges, double a, double b,
                        double c, uint64_t seed, int nplant, const double* plant) {
  if (!ctx || n < 1 || scale < 1 || scale > 31 || ((int64_t)1 << scale) < n || edges < 0 ||
      a < 0 || b < 0 || c < 0 || a + b + c > 1.0 || nplant < 0 || (nplant > 0 && !plant) ||
      n > INT32_MAX)
    return fail(ctx, RBL_ERR_INVALID, "rbl_gen_matrix_rmat: bad arguments");
  if (ctx->nranks > 16) return fail(ctx, RBL_ERR_INVALID, "rbl_gen_matrix_rmat: at most 16 ranks");
  HIPC(hipSetDevice(ctx->device));
  free_run(ctx);
  free_matrix(ctx);
  RmatParams p;
  p.n = n;
  p.scale = scale;
  p.edges = edges;
  p.a = a;
  p.b = b;
  p.c = c;
  p.seed = seed;
  p.relabel = ctx->relabel_opt != 0;
  if (p.relabel) p.perm = make_scatter(n, seed ^ kRelabelK);
  // degrees of every row (all ranks draw every edge): they size the key buffer and balance
  // the row split by nonzeros (R-MAT's low ids are its hubs)
  DevBuf<int32_t> d_deg;
  HIPC(d_deg.alloc(n));
  HIPC(hipMemsetAsync(d_deg, 0, n * sizeof(int32_t), ctx->stream));
  rmat_degree(p, d_deg, ctx->stream);
  HIPC(hipGetLastError());
  std::vector<int32_t> deg(n);
  HIPC(hipMemcpyAsync(deg.data(), d_deg, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  d_deg.reset();  // n degrees, before the CSR
  const int P = ctx->nranks;
  std::vector<int64_t> pre(n + 1, 0);  // nonzeros (with duplicates) + diagonal, prefix
  for (int64_t r = 0; r < n; ++r) pre[r + 1] = pre[r] + deg[r] + 1;
  ctx->bounds.assign(P + 1, 0);
  ctx->bounds[P] = n;
  for (int q = 1; q < P; ++q) {
    const int64_t target = pre[n] * q / P;
    ctx->bounds[q] = std::lower_bound(pre.begin(), pre.end(), target) - pre.begin();
    ctx->bounds[q] = std::max(ctx->bounds[q], ctx->bounds[q - 1]);
  }
  const int64_t r0 = ctx->bounds[ctx->rank], r1 = ctx->bounds[ctx->rank + 1], m = r1 - r0;
  ctx->n = n;
  ctx->r0 = r0;
  ctx->r1 = r1;
  ctx->nloc = m;
  int64_t own = 0;
  for (int64_t r = r0; r < r1; ++r) own += deg[r];
  DevBuf<double> d_plant;
  CHK(upload_plant(ctx, nplant, plant, d_plant));
  HIPC(ctx->d_rowptr.alloc(m + 1));
  int64_t nnz = 0;
  int32_t* col = nullptr;  // the generator allocates both: adopted whatever it returns
  double* val = nullptr;
  const int st = rmat_local_csr(p, r0, r1, own, nplant, d_plant, ctx->d_rowptr, &col, &val, &nnz,
                                ctx->stream);
  ctx->d_col.adopt(col);
  ctx->d_val.adopt(val);
  d_plant.reset();  // before the formats are built, so their allocations are placed as ever
  ctx->relabeled = p.relabel;
  ctx->relabel_perm = p.perm;
  if (st == -1) return fail(ctx, RBL_ERR_INVALID, "rbl_gen_matrix_rmat: > 2^31 keys on one rank");
  if (st < 0) return fail(ctx, st == -3 ? RBL_ERR_OOM : RBL_ERR_HIP, "rbl_gen_matrix_rmat: device generation failed");
  ctx->nnz = nnz;
  std::vector<int64_t> rp(m + 1);
  HIPC(hipMemcpy(rp.data(), ctx->d_rowptr, (m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  CHK(halo_from_footprint(ctx));
  CHK(prepare_window(ctx, rp));
  return setup_halo(ctx);
}

int rbl_set_matrix_normal(rbl_ctx* ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* ptr,
                          const int64_t* ind, const double* val, int index_base, int layout) {
  if (!ctx || nrows < 1 || ncols < 1 || nnz < 0 || !ptr || (nnz && (!ind || !val)) ||
      (index_base != 0 && index_base != 1) || (layout != 0 && layout != 1))
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: bad arguments");
  if (ctx->nranks > 1)  // before any collective: no rank waits for another
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: one rank only");
  if (nrows > INT32_MAX || ncols > INT32_MAX)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: nrows and ncols must be < 2^31 (int32 ids)");
  if (nnz >= INT32_MAX)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: nnz must be < 2^31 - 1 (the device transpose)");
  // the arrays passed are the CSR of side P: B's rows (layout 0) or B^T's rows (layout 1, B's CSC)
  const int P = layout;
  const int64_t rows = P == 0 ? nrows : ncols, ids = P == 0 ? ncols : nrows;
  if (ptr[rows] - ptr[0] != nnz || ptr[0] != index_base)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: ptr does not span nnz entries");
  std::vector<int64_t> rp(rows + 1);
  for (int64_t i = 0; i <= rows; ++i) {
    rp[i] = ptr[i] - index_base;
    if (rp[i] < (i ? rp[i - 1] : 0) || rp[i] > nnz)
      return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: ptr not monotone");
  }
  std::vector<int32_t> ci(std::max<int64_t>(nnz, 1));
  for (int64_t i = 0; i < rows; ++i)
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
      const int64_t c = ind[e] - index_base;
      if (c < 0 || c >= ids) return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: index out of range");
      // strictly ascending (canonical: sorted, no duplicates) — the transpose's per-row order and
      // its value lookup rely on it
      if (e > rp[i] && c <= ci[e - 1])
        return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_normal: indices must be strictly ascending "
                                          "within each row (layout 0) / column (layout 1)");
      ci[e] = (int32_t)c;
    }
  HIPC(hipSetDevice(ctx->device));
  free_run(ctx);
  free_matrix(ctx);
  ctx->bounds = {0, ncols};
  ctx->n = ncols;
  ctx->r0 = 0;
  ctx->r1 = ncols;
  ctx->nloc = ncols;
  ctx->nnz = nnz;
  ctx->rect = true;
  ctx->rect_m = nrows;
  const size_t ne = (size_t)std::max<int64_t>(nnz, 1);
  auto& S = ctx->rect_side[P];
  auto& T = ctx->rect_side[1 - P];
  HIPC(S.rowptr.alloc(rows + 1));
  HIPC(S.col.alloc(ne));
  HIPC(S.val.alloc(ne));
  HIPC(T.rowptr.alloc(ids + 1));
  HIPC(T.col.alloc(ne));
  HIPC(T.val.alloc(ne));
  HIPC(hipMemcpy(S.rowptr, rp.data(), (rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (nnz) {
    HIPC(hipMemcpy(S.col, ci.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(S.val, val, nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  // the other orientation on the device (count, scan, fill, per-row sort: spmm_rect.hip)
  const int te = rect_transpose(rows, ids, nnz, S.rowptr, S.col, S.val, T.rowptr, T.col, T.val, ctx->stream);
  if (te != 0)
    return fail(ctx, te == (int)hipErrorOutOfMemory ? RBL_ERR_OOM : RBL_ERR_HIP,
                std::string("rbl_set_matrix_normal: device transpose: ") + hipGetErrorString((hipError_t)te));
  std::vector<int64_t> tp(ids + 1);
  HIPC(hipMemcpy(tp.data(), T.rowptr, (ids + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (tp[ids] != nnz) return fail(ctx, RBL_ERR_HIP, "rbl_set_matrix_normal: device transpose lost entries");
  // the task tables of both orientations (64 doubles of scratch per segment slot: b <= 64 per launch)
  CHK(build_seg(ctx, rp, S, kRectSegLen, kRectPack, kWave));
  CHK(build_seg(ctx, tp, T, kRectSegLen, kRectPack, kWave));
  ctx->need_lo.assign(1, 0);
  ctx->need_hi.assign(1, 0);
  return setup_halo(ctx);
}

int rbl_set_matrix_kernel(rbl_ctx* ctx, int64_t n, int d, const double* X, int64_t ldx, int kind,
                          double gamma, double coef0, int degree) {
  if (!ctx || n < 1 || !X || ldx < n)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: bad arguments");
  if (ctx->nranks > 1)  // before any collective: no rank waits for another
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: one rank only");
  if (d < 1 || d > RBL_KERNOP_MAX_DIM)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: d must be in [1," +
                                          std::to_string(RBL_KERNOP_MAX_DIM) + "]");
  if (kind != RBL_KERNEL_RBF && kind != RBL_KERNEL_LAPLACE && kind != RBL_KERNEL_POLY)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: unknown kernel kind");
  if (!std::isfinite(gamma) || gamma <= 0.0 || !std::isfinite(coef0))
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: gamma must be finite and > 0, coef0 finite");
  if (degree < 1 || degree > 8)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: degree must be in [1,8]");
  const int d4 = 4 * ((d + 3) / 4);
  if (n >= ((int64_t)1 << 40) / RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: n too large");
  // column-major host points -> row-major, zero-padded to d4 columns
  std::vector<double> xr((size_t)n * d4, 0.0);
  for (int k = 0; k < d; ++k)
    for (int64_t i = 0; i < n; ++i) {
      const double v = X[i + k * ldx];
      if (!std::isfinite(v)) return fail(ctx, RBL_ERR_INVALID, "rbl_set_matrix_kernel: X has a non-finite entry");
      xr[(size_t)i * d4 + k] = v;
    }
  HIPC(hipSetDevice(ctx->device));
  free_run(ctx);
  free_matrix(ctx);
  ctx->bounds = {0, n};
  ctx->n = n;
  ctx->r0 = 0;
  ctx->r1 = n;
  ctx->nloc = n;
  ctx->nnz = n * n;
  ctx->kernop = true;
  ctx->kern_d = d;
  ctx->kern_d4 = d4;
  ctx->kern_kind = kind;
  ctx->kern_degree = degree;
  ctx->kern_gamma = gamma;
  ctx->kern_coef0 = coef0;
  HIPC(ctx->d_kern_x.alloc((size_t)n * d4));
  HIPC(ctx->d_kern_nrm.alloc((size_t)n));
  HIPC(hipMemcpyAsync(ctx->d_kern_x, xr.data(), (size_t)n * d4 * sizeof(double), hipMemcpyHostToDevice,
                      ctx->stream));
  kernop_norms(n, d4, ctx->d_kern_x, ctx->d_kern_nrm, ctx->stream);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->need_lo.assign(1, 0);
  ctx->need_hi.assign(1, 0);
  return setup_halo(ctx);
}

int rbl_set_kernel_scale(rbl_ctx* ctx, const double* scale, double nugget) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, "rbl_set_kernel_scale: no kernel matrix");
  if (!std::isfinite(nugget)) return fail(ctx, RBL_ERR_INVALID, "rbl_set_kernel_scale: nugget must be finite");
  for (int64_t i = 0; scale && i < ctx->n; ++i)
    if (!std::isfinite(scale[i]))
      return fail(ctx, RBL_ERR_INVALID, "rbl_set_kernel_scale: scale has a non-finite entry");
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));  // steps in flight still read the old scale
  if (!scale) {
    ctx->d_kern_scale.reset();
  } else {
    if (!ctx->d_kern_scale) HIPC(ctx->d_kern_scale.alloc((size_t)ctx->n));
    HIPC(hipMemcpy(ctx->d_kern_scale, scale, ctx->n * sizeof(double), hipMemcpyHostToDevice));
  }
  ctx->kern_nugget = nugget;
  return RBL_OK;
}

int rbl_kernel_info(rbl_ctx* ctx, int64_t* n, int* d, int* kind, double* gamma, double* coef0, int* degree,
                    int* has_scale, double* nugget) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, "rbl_kernel_info: no kernel matrix");
  if (n) *n = ctx->n;
  if (d) *d = ctx->kern_d;
  if (kind) *kind = ctx->kern_kind;
  if (gamma) *gamma = ctx->kern_gamma;
  if (coef0) *coef0 = ctx->kern_coef0;
  if (degree) *degree = ctx->kern_degree;
  if (has_scale) *has_scale = ctx->d_kern_scale ? 1 : 0;
  if (nugget) *nugget = ctx->kern_nugget;
  return RBL_OK;
}

int rbl_bench_kernel_pass(rbl_ctx* ctx, int b, int reps, double* ms) {
  if (!ctx || b < 1 || b > RBL_MAX_BLOCK || reps < 1 || !ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_pass: bad arguments");
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, "rbl_bench_kernel_pass: no kernel matrix");
  HIPC(hipSetDevice(ctx->device));
  DevBuf<double> q, u;
  HIPC(q.alloc((size_t)ctx->n * b));
  HIPC(u.alloc((size_t)ctx->n * b));
  randn_block(q, ctx->n, b, 0, 1, ctx->stream);
  const KernOp op = kernop(ctx);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  int st = RBL_OK;
  kernop_apply(op, q, b, u, ctx->stream);  // warm-up
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int r = 0; r < reps; ++r) kernop_apply(op, q, b, u, ctx->stream);
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float t = 0.f;
  if (hipEventElapsedTime(&t, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)t / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_kernel_pass: a HIP call failed");
  return RBL_OK;
}

namespace {
// The buffers of one cross-kernel product (rbl_kernel_cross, rbl_bench_kernel_cross): they live as
// long as the call — the new points row-major m x d4 with their norms, the two blocks, and the
// S x rows x b partials of a split column range (empty when S = 1).
struct CrossBufs {
  DevBuf<double> z, znrm, w, wr, y, part;
};

// Z (m x d, column-major, ldz) -> row-major m x d4 zero-padded; false at a non-finite entry
bool cross_points(int64_t m, int d, int d4, const double* Z, int64_t ldz, std::vector<double>& zr) {
  zr.assign((size_t)m * d4, 0.0);
  for (int k = 0; k < d; ++k)
    for (int64_t i = 0; i < m; ++i) {
      const double v = Z[i + k * ldz];
      if (!std::isfinite(v)) return false;
      zr[(size_t)i * d4 + k] = v;
    }
  return true;
}

// the product of the kernel matrix held with the m uploaded points B.z: trans = 0 kappa(Z, X) diag(s),
// trans = 1 diag(s) kappa(X, Z)
KernCross cross_op(const rbl_ctx* ctx, const CrossBufs& B, int64_t m, int trans) {
  KernCross op;
  op.d4 = ctx->kern_d4;
  op.kind = ctx->kern_kind;
  op.degree = ctx->kern_degree;
  op.gamma = ctx->kern_gamma;
  op.coef0 = ctx->kern_coef0;
  if (trans) {
    op.mr = ctx->n, op.R = ctx->d_kern_x, op.rnrm = ctx->d_kern_nrm, op.sr = ctx->d_kern_scale;
    op.mc = m, op.C = B.z, op.cnrm = B.znrm;
  } else {
    op.mr = m, op.R = B.z, op.rnrm = B.znrm;
    op.mc = ctx->n, op.C = ctx->d_kern_x, op.cnrm = ctx->d_kern_nrm, op.sc = ctx->d_kern_scale;
  }
  return op;
}
}  // namespace

int rbl_kernel_cross_splits(int64_t rows, int64_t cols, int d) {
  if (rows < 1 || cols < 1 || d < 1 || d > RBL_KERNOP_MAX_DIM) return RBL_ERR_INVALID;
  return kernop_cross_splits(rows, cols, 4 * ((d + 3) / 4));
}

int rbl_kernel_cross(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int trans, int b, const double* W,
                     int64_t ldw, double* Y, int64_t ldy) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, "rbl_kernel_cross: no kernel matrix");
  if (trans != 0 && trans != 1) return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_cross: trans must be 0 or 1");
  if (m < 1 || b < 1 || b > RBL_MAX_BLOCK || m >= ((int64_t)1 << 40) / RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_cross: m must be >= 1 and b in [1," +
                                          std::to_string(RBL_MAX_BLOCK) + "]");
  const int64_t n = ctx->n, wrows = trans ? m : n, yrows = trans ? n : m;
  if (!Z || !W || !Y || ldz < m || ldw < wrows || ldy < yrows)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_cross: NULL block or a leading dimension below its rows");
  const int d4 = ctx->kern_d4;
  std::vector<double> zr, wh((size_t)wrows * b);
  if (!cross_points(m, ctx->kern_d, d4, Z, ldz, zr))
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_cross: Z has a non-finite entry");
  for (int c = 0; c < b; ++c)
    for (int64_t i = 0; i < wrows; ++i) {
      const double v = W[i + c * ldw];
      if (!std::isfinite(v)) return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_cross: W has a non-finite entry");
      wh[(size_t)i + (size_t)c * wrows] = v;
    }
  HIPC(hipSetDevice(ctx->device));
  const int S = kernop_cross_splits(yrows, wrows, d4);
  CrossBufs B;
  HIPC(B.z.alloc((size_t)m * d4));
  HIPC(B.znrm.alloc((size_t)m));
  HIPC(B.w.alloc((size_t)std::max(wrows, yrows) * b));
  HIPC(B.wr.alloc((size_t)wrows * b));
  HIPC(B.y.alloc((size_t)yrows * b));
  if (S > 1) HIPC(B.part.alloc((size_t)S * yrows * b));
  HIPC(hipMemcpyAsync(B.z, zr.data(), zr.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  kernop_norms(m, d4, B.z, B.znrm, ctx->stream);
  HIPC(hipMemcpyAsync(B.w, wh.data(), wh.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  colmajor_to_rowmajor(B.w, wrows, b, B.wr, ctx->stream);
  if (!kernop_cross(cross_op(ctx, B, m, trans), B.wr, b, B.y, B.part, S, ctx->stream))
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_cross: shape out of range");
  HIPC(hipGetLastError());
  rowmajor_to_colmajor(B.y, yrows, b, B.w, ctx->stream);
  std::vector<double> yh((size_t)yrows * b);
  HIPC(hipMemcpyAsync(yh.data(), B.w, yh.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int c = 0; c < b; ++c) std::copy_n(yh.data() + (size_t)c * yrows, yrows, Y + c * ldy);
  return RBL_OK;
}

int rbl_bench_kernel_cross(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int trans, int b, int splits,
                           int reps, double* ms) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, "rbl_bench_kernel_cross: no kernel matrix");
  if (m < 1 || !Z || ldz < m || (trans != 0 && trans != 1) || b < 1 || b > RBL_MAX_BLOCK || reps < 1 || !ms ||
      splits < 0 || m >= ((int64_t)1 << 40) / RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_cross: bad arguments");
  const int64_t n = ctx->n, wrows = trans ? m : n, yrows = trans ? n : m;
  const int d4 = ctx->kern_d4;
  std::vector<double> zr;
  if (!cross_points(m, ctx->kern_d, d4, Z, ldz, zr))
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_cross: Z has a non-finite entry");
  HIPC(hipSetDevice(ctx->device));
  const int S = splits ? splits : kernop_cross_splits(yrows, wrows, d4);
  CrossBufs B;
  HIPC(B.z.alloc((size_t)m * d4));
  HIPC(B.znrm.alloc((size_t)m));
  HIPC(B.wr.alloc((size_t)wrows * b));
  HIPC(B.y.alloc((size_t)yrows * b));
  if (S > 1) HIPC(B.part.alloc((size_t)S * yrows * b));
  HIPC(hipMemcpyAsync(B.z, zr.data(), zr.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  kernop_norms(m, d4, B.z, B.znrm, ctx->stream);
  randn_block(B.wr, wrows, b, 0, 1, ctx->stream);
  const KernCross op = cross_op(ctx, B, m, trans);
  if (!kernop_cross(op, B.wr, b, B.y, B.part, S, ctx->stream))  // warm-up
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_cross: splits out of range for this shape");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  int st = RBL_OK;
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int r = 0; r < reps; ++r) kernop_cross(op, B.wr, b, B.y, B.part, S, ctx->stream);
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float t = 0.f;
  if (hipEventElapsedTime(&t, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)t / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_kernel_cross: a HIP call failed");
  return RBL_OK;
}

namespace {
static_assert(RBL_KNN_MAX == kKernKnnMax, "rbl_hip.h and kernels.hpp name the same largest k");

// The buffers of one neighbour search (rbl_kernel_knn, rbl_bench_kernel_knn): they live as long as
// the call — the new points row-major m x d4 with their norms (cross mode), the lists rows x k
// row-major, and the splits' lists (empty when S = 1).
struct KnnBufs {
  DevBuf<double> z, znrm, d2, part_d2;
  DevBuf<int32_t> idx, part_idx;
};

// what both entries check, in one order; on RBL_OK zr holds the row-major points of Z (cross mode)
// and S the splits to use
int knn_check(rbl_ctx* ctx, const char* who, int64_t m, const double* Z, int64_t ldz, int k, int splits,
              std::vector<double>& zr, int& S) {
  const std::string w(who);
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, w + ": no kernel matrix");
  const int64_t n = ctx->n;
  if (Z ? (m < 1 || ldz < m || m >= ((int64_t)1 << 40) / RBL_MAX_BLOCK) : m != 0)
    return fail(ctx, RBL_ERR_INVALID, w + ": m must be >= 1 with Z (ldz >= m) and 0 without");
  if (k < 1 || k > RBL_KNN_MAX || k > (Z ? n : n - 1))
    return fail(ctx, RBL_ERR_INVALID, w + ": k must be in [1," + std::to_string(RBL_KNN_MAX) +
                                          "] and at most the column points available");
  if (n > (int64_t)INT32_MAX - 64) return fail(ctx, RBL_ERR_INVALID, w + ": n too large for int32 indices");
  const int d4 = ctx->kern_d4;
  const int64_t rows = Z ? m : n;
  if (splits < 0 || splits > kKernCrossMaxSplits)   // (beyond the stages: kernop_knn refuses)
    return fail(ctx, RBL_ERR_INVALID, w + ": splits must be 0 (the rule) or in [1,64]");
  if (Z && !cross_points(m, ctx->kern_d, d4, Z, ldz, zr))
    return fail(ctx, RBL_ERR_INVALID, w + ": Z has a non-finite entry");
  S = splits ? splits : kernop_cross_splits(rows, n, d4);
  return RBL_OK;
}

// allocate, upload Z (cross mode) and describe the search
int knn_setup(rbl_ctx* ctx, int64_t m, bool cross, int k, int S, const std::vector<double>& zr, KnnBufs& B,
              KernKnn& op) {
  const int64_t n = ctx->n, rows = cross ? m : n;
  const int d4 = ctx->kern_d4;
  HIPC(B.idx.alloc((size_t)rows * k));
  HIPC(B.d2.alloc((size_t)rows * k));
  if (S > 1) {
    HIPC(B.part_idx.alloc((size_t)S * rows * k));
    HIPC(B.part_d2.alloc((size_t)S * rows * k));
  }
  op.mr = rows, op.mc = n, op.d4 = d4, op.k = k, op.self = !cross;
  op.C = ctx->d_kern_x, op.cnrm = ctx->d_kern_nrm;
  if (cross) {
    HIPC(B.z.alloc((size_t)m * d4));
    HIPC(B.znrm.alloc((size_t)m));
    HIPC(hipMemcpyAsync(B.z, zr.data(), zr.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    kernop_norms(m, d4, B.z, B.znrm, ctx->stream);
    op.R = B.z, op.rnrm = B.znrm;
  } else {
    op.R = ctx->d_kern_x, op.rnrm = ctx->d_kern_nrm;
  }
  return RBL_OK;
}
}  // namespace

int rbl_kernel_knn(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int k, int splits, int32_t* idx,
                   int64_t ldi, double* d2, int64_t ldd) {
  if (!ctx) return RBL_ERR_INVALID;
  std::vector<double> zr;
  int S = 1;
  CHK(knn_check(ctx, "rbl_kernel_knn", m, Z, ldz, k, splits, zr, S));
  const int64_t rows = Z ? m : ctx->n;
  if (!idx || !d2 || ldi < rows || ldd < rows)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_knn: NULL output or a leading dimension below its rows");
  HIPC(hipSetDevice(ctx->device));
  KnnBufs B;
  KernKnn op;
  CHK(knn_setup(ctx, m, Z != nullptr, k, S, zr, B, op));
  if (!kernop_knn(op, B.idx, B.d2, B.part_idx, B.part_d2, S, ctx->stream))
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_knn: splits beyond the stages of the column range, or n too large");
  HIPC(hipGetLastError());
  std::vector<int32_t> ih((size_t)rows * k);
  std::vector<double> dh((size_t)rows * k);
  HIPC(hipMemcpyAsync(ih.data(), B.idx, ih.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(dh.data(), B.d2, dh.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int c = 0; c < k; ++c)   // row-major lists -> the caller's column-major blocks
    for (int64_t i = 0; i < rows; ++i) {
      idx[i + c * ldi] = ih[(size_t)i * k + c];
      d2[i + c * ldd] = dh[(size_t)i * k + c];
    }
  return RBL_OK;
}

int rbl_bench_kernel_knn(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int k, int splits, int reps,
                         double* ms) {
  if (!ctx) return RBL_ERR_INVALID;
  std::vector<double> zr;
  int S = 1;
  CHK(knn_check(ctx, "rbl_bench_kernel_knn", m, Z, ldz, k, splits, zr, S));
  if (reps < 1 || !ms) return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_knn: reps must be >= 1 and ms not NULL");
  HIPC(hipSetDevice(ctx->device));
  KnnBufs B;
  KernKnn op;
  CHK(knn_setup(ctx, m, Z != nullptr, k, S, zr, B, op));
  if (!kernop_knn(op, B.idx, B.d2, B.part_idx, B.part_d2, S, ctx->stream))  // warm-up
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_knn: splits beyond the stages of the column range, or n too large");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  int st = RBL_OK;
#ifdef RBL_KNN_COUNT
  unsigned long long cnt[2] = {0, 0};
  if (hipStreamSynchronize(ctx->stream) != hipSuccess || !kernop_knn_counts(cnt, true)) st = RBL_ERR_HIP;
#endif
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int r = 0; r < reps; ++r) kernop_knn(op, B.idx, B.d2, B.part_idx, B.part_d2, S, ctx->stream);
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float t = 0.f;
  if (hipEventElapsedTime(&t, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)t / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
#ifdef RBL_KNN_COUNT
  if (st == RBL_OK && kernop_knn_counts(cnt, false))
    fprintf(stderr, "rbl_bench_kernel_knn: %llu wave tiles per launch, %llu with an insertion\n",
            cnt[0] / reps, cnt[1] / reps);
#endif
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_kernel_knn: a HIP call failed");
  return RBL_OK;
}

// ---- partial pivoted Cholesky of the kernel matrix (pchol.hip) --------------------------------------
namespace {
static_assert(RBL_PCHOL_MAX_RANK == kPcholMaxRank, "rbl_hip.h and kernels.hpp name the same largest rank");

// The buffers of one factorisation (rbl_kernel_pchol, rbl_bench_kernel_pchol): they live as long as
// the call — L column-major n x R, the residual diagonal, the slabs' partials (two buffers) and the
// small records (trace R + 1 and the floor; piv R, the rank and the R + 2 stop flags).
struct PcholBufs {
  DevBuf<double> L, d, part, rec;
  DevBuf<int32_t> pidx, irec;
};

// what both entries check, in one order, before anything is allocated
int pchol_check(rbl_ctx* ctx, const char* who, int max_rank, double tol) {
  const std::string w(who);
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, w + ": no kernel matrix");
  if (max_rank < 1 || max_rank > RBL_PCHOL_MAX_RANK || max_rank > ctx->n)
    return fail(ctx, RBL_ERR_INVALID, w + ": max_rank must be in [1, min(n, " + std::to_string(RBL_PCHOL_MAX_RANK) + ")]");
  if (!std::isfinite(tol) || tol < 0.0 || tol >= 1.0)
    return fail(ctx, RBL_ERR_INVALID, w + ": tol must be finite and in [0, 1)");
  if (ctx->n > (int64_t)INT32_MAX - 64) return fail(ctx, RBL_ERR_INVALID, w + ": n too large for int32 indices");
  return RBL_OK;
}

int pchol_setup(rbl_ctx* ctx, int R, PcholBufs& B, PcholWork& W) {
  const int64_t n = ctx->n;
  const size_t G = (size_t)pchol_slabs(n);
  HIPC(B.L.alloc((size_t)n * R));
  HIPC(B.d.alloc((size_t)n));
  HIPC(B.part.alloc(4 * G));
  HIPC(B.pidx.alloc(2 * G));
  HIPC(B.rec.alloc((size_t)R + 2));
  HIPC(B.irec.alloc((size_t)2 * R + 3));
  W.L = B.L, W.ldl = n, W.d = B.d;
  W.pmax = B.part, W.ptrace = B.part + 2 * G, W.pidx = B.pidx;
  W.trace = B.rec, W.floor_ = B.rec + R + 1;
  W.piv = B.irec, W.rank = B.irec + R, W.flag = B.irec + R + 1;
  return RBL_OK;
}
}  // namespace

int rbl_kernel_pchol(rbl_ctx* ctx, int max_rank, double tol, double* L, int64_t ldl, int32_t* piv, double* trace,
                     int* rank_out) {
  if (!ctx) return RBL_ERR_INVALID;
  CHK(pchol_check(ctx, "rbl_kernel_pchol", max_rank, tol));
  const int64_t n = ctx->n;
  if (L && ldl < n) return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_pchol: ldl must be >= n");
  HIPC(hipSetDevice(ctx->device));
  const int R = max_rank;
  PcholBufs B;
  PcholWork W;
  CHK(pchol_setup(ctx, R, B, W));
  if (!kernop_pchol(kernop(ctx), R, tol, W, ctx->stream))
    return fail(ctx, RBL_ERR_HIP, "rbl_kernel_pchol: the factorisation could not be enqueued");
  HIPC(hipGetLastError());
  std::vector<double> th((size_t)R + 1);
  std::vector<int32_t> ih((size_t)R + 1);  // piv, then the rank
  HIPC(hipMemcpyAsync(th.data(), W.trace, th.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(ih.data(), W.piv, ih.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (L) HIPC(hipMemcpy2DAsync(L, (size_t)ldl * sizeof(double), W.L, (size_t)n * sizeof(double),
                               (size_t)n * sizeof(double), (size_t)R, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  const int rank = ih[R];
  if (rank < 0 || rank > R) return fail(ctx, RBL_ERR_HIP, "rbl_kernel_pchol: the device reported no rank");
  if (piv) std::copy_n(ih.data(), R, piv);
  if (trace)
    for (int j = 0; j <= R; ++j) trace[j] = th[std::min(j, rank)];
  if (rank_out) *rank_out = rank;
  return RBL_OK;
}

int rbl_bench_kernel_pchol(rbl_ctx* ctx, int max_rank, int reps, double* ms) {
  if (!ctx) return RBL_ERR_INVALID;
  CHK(pchol_check(ctx, "rbl_bench_kernel_pchol", max_rank, 0.0));
  if (reps < 1 || !ms) return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_pchol: reps must be >= 1 and ms not NULL");
  HIPC(hipSetDevice(ctx->device));
  PcholBufs B;
  PcholWork W;
  CHK(pchol_setup(ctx, max_rank, B, W));
  const KernOp op = kernop(ctx);
  if (!kernop_pchol(op, max_rank, 0.0, W, ctx->stream))  // warm-up
    return fail(ctx, RBL_ERR_HIP, "rbl_bench_kernel_pchol: the factorisation could not be enqueued");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return fail(ctx, RBL_ERR_HIP, "rbl_bench_kernel_pchol: hipEventCreate failed");
  }
  int st = RBL_OK;
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int r = 0; r < reps; ++r)
    if (!kernop_pchol(op, max_rank, 0.0, W, ctx->stream)) st = RBL_ERR_HIP;
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float t = 0.f;
  if (hipEventElapsedTime(&t, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)t / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_kernel_pchol: a HIP call failed");
  return RBL_OK;
}

// ---- k-means (kmeans.hip): the points live in the context, beside whatever matrix it holds ---------
namespace {
static_assert(RBL_KMEANS_MAX_CLUSTERS == kKmeansMaxClusters, "rbl_hip.h and kernels.hpp name the same largest c");

// The buffers of one Lloyd run (rbl_kmeans_run, rbl_bench_kmeans_iter): they live as long as the call —
// the two centre arrays (C_t and C_{t+1}) with their norms, the two label arrays (labels_t and
// labels_{t-1}), d2(i, label_i), the slabs' records, the reduced record and the decision record.
struct KmeansBufs {
  DevBuf<double> cen[2], cnrm[2], dmin, part, tot, rec;
  DevBuf<int32_t> lab[2];
};

void km_points(const rbl_ctx* ctx, KmeansPoints& P) {
  P.n = ctx->km_n, P.d4 = ctx->km_d4, P.X = ctx->d_km_x, P.nrm = ctx->d_km_nrm;
}

// what rbl_kmeans_run and the bench hook check, in one order; on RBL_OK cr holds C0 row-major c x d4
int km_check(rbl_ctx* ctx, const char* who, int c, const double* C0, int64_t ldc0, std::vector<double>& cr) {
  const std::string w(who);
  if (ctx->km_n == 0) return fail(ctx, RBL_ERR_STATE, w + ": no points set (rbl_kmeans_set_points)");
  if (c < 1 || c > RBL_KMEANS_MAX_CLUSTERS || c > ctx->km_n)
    return fail(ctx, RBL_ERR_INVALID, w + ": c must be in [1," + std::to_string(RBL_KMEANS_MAX_CLUSTERS) +
                                          "] and at most n");
  if (!C0 || ldc0 < c) return fail(ctx, RBL_ERR_INVALID, w + ": NULL centres or ldc0 < c");
  if (!cross_points(c, ctx->km_d, ctx->km_d4, C0, ldc0, cr))
    return fail(ctx, RBL_ERR_INVALID, w + ": a centre has a non-finite entry");
  return RBL_OK;
}

int km_setup(rbl_ctx* ctx, int c, const std::vector<double>& cr, KmeansBufs& B, KmeansGeometry& g) {
  const int64_t n = ctx->km_n;
  const int d4 = ctx->km_d4;
  g = kmeans_geometry(n, d4, c);
  for (int k = 0; k < 2; ++k) {
    HIPC(B.cen[k].alloc((size_t)c * d4));
    HIPC(B.cnrm[k].alloc((size_t)c));
    HIPC(B.lab[k].alloc((size_t)n));
  }
  HIPC(B.dmin.alloc((size_t)n));
  HIPC(B.part.alloc((size_t)g.slabs * g.len));
  HIPC(B.tot.alloc((size_t)g.len));
  HIPC(B.rec.alloc(3));
  HIPC(hipMemcpyAsync(B.cen[0], cr.data(), cr.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  kernop_norms(c, d4, B.cen[0], B.cnrm[0], ctx->stream);
  kmeans_fill_labels(n, -1, B.lab[1], ctx->stream);   // "labels_{-1}": every label of t = 0 counts as changed
  return RBL_OK;
}

// iteration t against the centres in slot cur: labels into lab[t & 1], the record, C_{t+1} into the other slot
bool km_iteration(rbl_ctx* ctx, int c, KmeansBufs& B, int t, int cur) {
  KmeansPoints P;
  km_points(ctx, P);
  if (!kmeans_assign(P, c, B.cen[cur], B.cnrm[cur], B.lab[t & 1], B.dmin, ctx->stream)) return false;
  if (!kmeans_update(P, c, B.lab[t & 1], B.lab[(t + 1) & 1], B.dmin, B.part, B.tot, ctx->stream)) return false;
  kmeans_form(c, P.d4, B.tot, B.cen[cur], B.cen[cur ^ 1], B.cnrm[cur ^ 1], B.rec, ctx->stream);
  return true;
}
}  // namespace

int rbl_kmeans_set_points(rbl_ctx* ctx, int64_t n, int d, const double* X, int64_t ldx) {
  if (!ctx) return RBL_ERR_INVALID;
  if (n < 1 || n > (int64_t)INT32_MAX - 64 || d < 1 || d > RBL_KERNOP_MAX_DIM)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_set_points: n must be in [1, 2^31 - 65] and d in [1," +
                                          std::to_string(RBL_KERNOP_MAX_DIM) + "]");
  if (!X || ldx < n) return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_set_points: NULL points or ldx < n");
  const int d4 = 4 * ((d + 3) / 4);
  std::vector<double> xr;
  if (!cross_points(n, d, d4, X, ldx, xr))
    return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_set_points: X has a non-finite entry");
  HIPC(hipSetDevice(ctx->device));
  DevBuf<double> x, nrm;   // the context changes only once everything has succeeded
  HIPC(x.alloc((size_t)n * d4));
  HIPC(nrm.alloc((size_t)n));
  HIPC(hipStreamSynchronize(ctx->stream));
  HIPC(hipMemcpy(x, xr.data(), xr.size() * sizeof(double), hipMemcpyHostToDevice));
  kernop_norms(n, d4, x, nrm, ctx->stream);
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->d_km_x = std::move(x);
  ctx->d_km_nrm = std::move(nrm);
  ctx->km_n = n, ctx->km_d = d, ctx->km_d4 = d4;
  return RBL_OK;
}

int rbl_kmeans_clear(rbl_ctx* ctx) {
  if (!ctx) return RBL_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->d_km_x.reset();
  ctx->d_km_nrm.reset();
  ctx->km_n = 0, ctx->km_d = ctx->km_d4 = 0;
  return RBL_OK;
}

int rbl_kmeans_seed(rbl_ctx* ctx, int c, const double* uniforms, int32_t* picked_out) {
  if (!ctx) return RBL_ERR_INVALID;
  if (ctx->km_n == 0) return fail(ctx, RBL_ERR_STATE, "rbl_kmeans_seed: no points set (rbl_kmeans_set_points)");
  const int64_t n = ctx->km_n;
  if (c < 1 || c > RBL_KMEANS_MAX_CLUSTERS || c > n)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_seed: c must be in [1," + std::to_string(RBL_KMEANS_MAX_CLUSTERS) +
                                          "] and at most n");
  if (!uniforms || !picked_out) return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_seed: NULL uniforms or output");
  for (int r = 0; r < c; ++r)
    if (!std::isfinite(uniforms[r]) || uniforms[r] < 0.0 || uniforms[r] >= 1.0)
      return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_seed: every uniform must be finite and in [0, 1)");
  HIPC(hipSetDevice(ctx->device));
  DevBuf<double> dnew, w, slabtot;
  DevBuf<int32_t> picked;
  HIPC(dnew.alloc((size_t)n));
  HIPC(w.alloc((size_t)n));
  HIPC(slabtot.alloc((size_t)kmeans_seed_slabs(n)));
  HIPC(picked.alloc((size_t)c));
  std::vector<int32_t> ph((size_t)c);
  ph[0] = (int32_t)std::min<int64_t>((int64_t)std::floor(uniforms[0] * (double)n), n - 1);
  HIPC(hipMemcpyAsync(picked, ph.data(), sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  KmeansPoints P;
  km_points(ctx, P);
  for (int r = 1; r < c; ++r) {   // the host reads one index per round: the next round's centre
    if (!kmeans_seed_round(P, r, ph[r - 1], uniforms[r], dnew, w, slabtot, picked, ctx->stream))
      return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_seed: shape out of range");
    HIPC(hipMemcpyAsync(&ph[r], picked + r, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    if (ph[r] < 0 || ph[r] >= n) return fail(ctx, RBL_ERR_HIP, "rbl_kmeans_seed: a pick out of range");
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  HIPC(hipGetLastError());
  std::copy(ph.begin(), ph.end(), picked_out);
  return RBL_OK;
}

int rbl_kmeans_run(rbl_ctx* ctx, int c, const double* C0, int64_t ldc0, int max_iter, double tol,
                   int32_t* labels_out, double* centers_out, int64_t ldc, int64_t* counts_out, double* inertia_out,
                   int* n_iter_out, int* converged_out) {
  if (!ctx) return RBL_ERR_INVALID;
  std::vector<double> cr;
  CHK(km_check(ctx, "rbl_kmeans_run", c, C0, ldc0, cr));
  if (max_iter < 0) return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_run: max_iter must be >= 0");
  if (!std::isfinite(tol) || tol < 0.0) return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_run: tol must be finite and >= 0");
  if (centers_out && ldc < c) return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_run: ldc < c");
  HIPC(hipSetDevice(ctx->device));
  const int64_t n = ctx->km_n;
  const int d = ctx->km_d, d4 = ctx->km_d4;
  KmeansBufs B;
  KmeansGeometry g;
  CHK(km_setup(ctx, c, cr, B, g));
  int t = 0, cur = 0, conv = 0;
  double rec[3] = {0.0, 0.0, 0.0}, shift_prev = 0.0;
  for (;; ++t, cur ^= 1) {
    if (!km_iteration(ctx, c, B, t, cur)) return fail(ctx, RBL_ERR_INVALID, "rbl_kmeans_run: shape out of range");
    // the decision record of iteration t: the one thing the host reads inside the loop
    HIPC(hipMemcpyAsync(rec, B.rec, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(hipGetLastError());
    if (t >= 1 && rec[1] == 0.0) {
      conv = 1;
      break;
    }
    if (t >= 1 && tol > 0.0 && shift_prev <= tol) {   // |C_t - C_{t-1}|_F^2, formed with C_t
      conv = 2;
      break;
    }
    if (t == max_iter) break;
    shift_prev = rec[2];
  }
  // the consistent triple (labels_t, C_t, inertia_t) with counts_t
  std::vector<double> ch((size_t)c * d4), cnt((size_t)c);
  HIPC(hipMemcpyAsync(ch.data(), B.cen[cur], ch.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(cnt.data(), B.tot + (size_t)c * d4, (size_t)c * sizeof(double), hipMemcpyDeviceToHost,
                      ctx->stream));
  if (labels_out)
    HIPC(hipMemcpyAsync(labels_out, B.lab[t & 1], (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int k = 0; centers_out && k < d; ++k)
    for (int j = 0; j < c; ++j) centers_out[j + k * ldc] = ch[(size_t)j * d4 + k];
  for (int j = 0; counts_out && j < c; ++j) counts_out[j] = (int64_t)cnt[j];
  if (inertia_out) *inertia_out = rec[0];
  if (n_iter_out) *n_iter_out = t;
  if (converged_out) *converged_out = conv;
  return RBL_OK;
}

int rbl_bench_kmeans_iter(rbl_ctx* ctx, int c, const double* C0, int64_t ldc0, int reps, double* ms) {
  if (!ctx) return RBL_ERR_INVALID;
  std::vector<double> cr;
  CHK(km_check(ctx, "rbl_bench_kmeans_iter", c, C0, ldc0, cr));
  if (reps < 1 || !ms) return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kmeans_iter: reps must be >= 1 and ms not NULL");
  HIPC(hipSetDevice(ctx->device));
  KmeansBufs B;
  KmeansGeometry g;
  CHK(km_setup(ctx, c, cr, B, g));
  if (!km_iteration(ctx, c, B, 0, 0))  // warm-up
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kmeans_iter: shape out of range");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  int st = RBL_OK;
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int r = 0; r < reps; ++r) km_iteration(ctx, c, B, r + 1, 0);   // every iteration against C0
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float t = 0.f;
  if (hipEventElapsedTime(&t, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)t / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_kmeans_iter: a HIP call failed");
  return RBL_OK;
}

namespace {
// The buffers of one derivative product (rbl_kernel_hadamard, rbl_bench_kernel_hadamard): they live
// as long as the call — the two factors row-major n x r4 (zero-padded columns), the block and the
// result row-major, and one column-major image for the transposes.
struct HadamardBufs {
  DevBuf<double> a, b, q, qr, u;
};
static_assert(RBL_KWEIGHT_VALUE == kKernWeightValue && RBL_KWEIGHT_DGAMMA == kKernWeightDgamma &&
                  RBL_KWEIGHT_DSCALE == kKernWeightDscale,
              "rbl_hip.h and kernels.hpp name the same weights");

bool hadamard_mode_ok(int mode) {
  return mode == RBL_KWEIGHT_VALUE || mode == RBL_KWEIGHT_DGAMMA || mode == RBL_KWEIGHT_DSCALE;
}
// F (n x r, column-major, ldf) -> row-major n x r4 zero-padded; false at a non-finite entry
bool hadamard_factor(int64_t n, int r, int r4, const double* F, int64_t ldf, std::vector<double>& fr) {
  fr.assign((size_t)n * r4, 0.0);
  for (int k = 0; k < r; ++k)
    for (int64_t i = 0; i < n; ++i) {
      const double v = F[i + k * ldf];
      if (!std::isfinite(v)) return false;
      fr[(size_t)i * r4 + k] = v;
    }
  return true;
}
}  // namespace

int rbl_kernel_hadamard(rbl_ctx* ctx, int mode, int r, const double* A, int64_t lda, const double* B, int64_t ldb,
                        int b, const double* Q, int64_t ldq, double* U, int64_t ldu) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, "rbl_kernel_hadamard: no kernel matrix");
  if (!hadamard_mode_ok(mode)) return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_hadamard: unknown weight mode");
  const int d4 = ctx->kern_d4;
  if (r < 1 || r > RBL_KERNOP_MAX_DIM || d4 + 4 * ((r + 3) / 4) > RBL_KERNOP_MAX_DIM)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_hadamard: r must be >= 1 with 4 ceil(d / 4) + 4 ceil(r / 4) <= " +
                                          std::to_string(RBL_KERNOP_MAX_DIM));
  if (b < 1 || b > RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_hadamard: b must be in [1," + std::to_string(RBL_MAX_BLOCK) + "]");
  const int64_t n = ctx->n;
  if (!A || !B || !Q || !U || lda < n || ldb < n || ldq < n || ldu < n)
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_hadamard: NULL block or a leading dimension below n");
  const int r4 = 4 * ((r + 3) / 4);
  std::vector<double> ar, br, qh((size_t)n * b);
  if (!hadamard_factor(n, r, r4, A, lda, ar) || !hadamard_factor(n, r, r4, B, ldb, br))
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_hadamard: A or B has a non-finite entry");
  for (int c = 0; c < b; ++c)
    for (int64_t i = 0; i < n; ++i) {
      const double v = Q[i + c * ldq];
      if (!std::isfinite(v)) return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_hadamard: Q has a non-finite entry");
      qh[(size_t)i + (size_t)c * n] = v;
    }
  HIPC(hipSetDevice(ctx->device));
  HadamardBufs H;
  HIPC(H.a.alloc((size_t)n * r4));
  HIPC(H.b.alloc((size_t)n * r4));
  HIPC(H.q.alloc((size_t)n * b));
  HIPC(H.qr.alloc((size_t)n * b));
  HIPC(H.u.alloc((size_t)n * b));
  HIPC(hipMemcpyAsync(H.a, ar.data(), ar.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(H.b, br.data(), br.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(H.q, qh.data(), qh.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  colmajor_to_rowmajor(H.q, n, b, H.qr, ctx->stream);
  if (!kernop_hadamard(kernop(ctx), mode, r4, H.a, H.b, H.qr, b, H.u, ctx->stream))
    return fail(ctx, RBL_ERR_INVALID, "rbl_kernel_hadamard: shape out of range");
  HIPC(hipGetLastError());
  rowmajor_to_colmajor(H.u, n, b, H.q, ctx->stream);
  HIPC(hipMemcpyAsync(qh.data(), H.q, qh.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (int c = 0; c < b; ++c) std::copy_n(qh.data() + (size_t)c * n, n, U + c * ldu);
  return RBL_OK;
}

int rbl_bench_kernel_hadamard(rbl_ctx* ctx, int mode, int r, int b, int reps, double* ms) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->kernop) return fail(ctx, RBL_ERR_STATE, "rbl_bench_kernel_hadamard: no kernel matrix");
  const int d4 = ctx->kern_d4;
  if (!hadamard_mode_ok(mode) || r < 1 || r > RBL_KERNOP_MAX_DIM || d4 + 4 * ((r + 3) / 4) > RBL_KERNOP_MAX_DIM ||
      b < 1 || b > RBL_MAX_BLOCK || reps < 1 || !ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_hadamard: bad arguments");
  const int64_t n = ctx->n;
  const int r4 = 4 * ((r + 3) / 4);
  HIPC(hipSetDevice(ctx->device));
  HadamardBufs H;
  HIPC(H.a.alloc((size_t)n * r4));
  HIPC(H.b.alloc((size_t)n * r4));
  HIPC(H.qr.alloc((size_t)n * b));
  HIPC(H.u.alloc((size_t)n * b));
  // N(0,1) in every column, the padded ones included: the time does not depend on the values
  randn_block(H.a, n, r4, 0, 1, ctx->stream);
  randn_block(H.b, n, r4, 0, 2, ctx->stream);
  randn_block(H.qr, n, b, 0, 3, ctx->stream);
  const KernOp op = kernop(ctx);
  if (!kernop_hadamard(op, mode, r4, H.a, H.b, H.qr, b, H.u, ctx->stream))  // warm-up
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_kernel_hadamard: shape out of range");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  int st = RBL_OK;
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int k = 0; k < reps; ++k) kernop_hadamard(op, mode, r4, H.a, H.b, H.qr, b, H.u, ctx->stream);
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float t = 0.f;
  if (hipEventElapsedTime(&t, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)t / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_kernel_hadamard: a HIP call failed");
  return RBL_OK;
}

int rbl_rect_info(rbl_ctx* ctx, int64_t* nrows, int64_t* ncols, int64_t* nnz) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->rect) return fail(ctx, RBL_ERR_STATE, "rbl_rect_info: no rectangular matrix");
  if (nrows) *nrows = ctx->rect_m;
  if (ncols) *ncols = ctx->n;
  if (nnz) *nnz = ctx->nnz;
  return RBL_OK;
}

int rbl_get_matrix_rect(rbl_ctx* ctx, int trans, int64_t* rowptr, int32_t* colind, double* val) {
  if (!ctx || (trans != 0 && trans != 1)) return fail(ctx, RBL_ERR_INVALID, "rbl_get_matrix_rect: bad arguments");
  if (!ctx->rect) return fail(ctx, RBL_ERR_STATE, "rbl_get_matrix_rect: no rectangular matrix");
  HIPC(hipSetDevice(ctx->device));
  const auto& T = ctx->rect_side[trans];
  const int64_t rows = trans ? ctx->n : ctx->rect_m;
  if (rowptr) HIPC(hipMemcpy(rowptr, T.rowptr, (rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (colind && ctx->nnz)
    HIPC(hipMemcpy(colind, T.col, ctx->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (val && ctx->nnz) HIPC(hipMemcpy(val, T.val, ctx->nnz * sizeof(double), hipMemcpyDeviceToHost));
  return RBL_OK;
}

namespace {
// Y (rows of side `trans`) = side X (* scale per column), host column-major blocks of w columns.
// shifted (and a shift set): side is C = B - u v^T or C^T, i.e. Y = B X - u (v^T X) or
// Y = B^T X - v (u^T X), the b-vector reduced on the device, the shift before the scale.
static int rect_apply_host(rbl_ctx* ctx, int trans, int w, const double* X, double* Y, const double* scale,
                           bool shifted = false) {
  const int64_t rin = trans ? ctx->rect_m : ctx->n, rout = trans ? ctx->n : ctx->rect_m;
  shifted = shifted && ctx->rect_shift;
  const double* sa = !shifted ? nullptr : trans ? ctx->d_shift_v : ctx->d_shift_u;    // per output row
  const double* sin = !shifted ? nullptr : trans ? ctx->d_shift_u : ctx->d_shift_v;   // per input row
  DevBuf<double> x, xr, y, sc, sw, part;
  if (shifted) {
    HIPC(sw.alloc(w));
    HIPC(part.alloc((size_t)rect_colsum_grid(rin, w) * w));
  }
  const int64_t rmax = std::max(rin, rout);
  HIPC(x.alloc(rmax * w));
  HIPC(xr.alloc(rin * w));
  HIPC(y.alloc(rout * w));
  if (scale) {
    HIPC(sc.alloc(w));
    HIPC(hipMemcpyAsync(sc, scale, w * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  HIPC(hipMemcpyAsync(x, X, rin * w * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  colmajor_to_rowmajor(x, rin, w, xr, ctx->stream);
  {
    StageScope t(ctx, RBL_STAGE_AQ);
    if (shifted) rect_colsum(rin, w, sin, xr, part, sw, ctx->stream);
    spmm_rect(rect_tier(ctx, trans), xr, w, y, nullptr, nullptr, sc, ctx->stream, sa,
              sw);
  }
  HIPC(hipGetLastError());
  rowmajor_to_colmajor(y, rout, w, x, ctx->stream);
  HIPC(hipMemcpyAsync(Y, x, rout * w * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  return RBL_OK;
}
}  // namespace

int rbl_apply_rect(rbl_ctx* ctx, int trans, int b, const double* X, double* Y) {
  if (!ctx || (trans != 0 && trans != 1) || b < 1 || b > RBL_MAX_BLOCK || !X || !Y)
    return fail(ctx, RBL_ERR_INVALID, "rbl_apply_rect: bad arguments");
  if (!ctx->rect) return fail(ctx, RBL_ERR_STATE, "rbl_apply_rect: no rectangular matrix");
  HIPC(hipSetDevice(ctx->device));
  return rect_apply_host(ctx, trans, b, X, Y, nullptr);
}

int rbl_left_vectors(rbl_ctx* ctx, int k, const double* V, const double* sigma, double* U_out) {
  if (!ctx || k < 1 || k > RBL_MAX_BLOCK || !V || !sigma || !U_out)
    return fail(ctx, RBL_ERR_INVALID, "rbl_left_vectors: bad arguments");
  if (!ctx->rect) return fail(ctx, RBL_ERR_STATE, "rbl_left_vectors: no rectangular matrix");
  HIPC(hipSetDevice(ctx->device));
  std::vector<double> inv(k);
  for (int j = 0; j < k; ++j) inv[j] = 1.0 / sigma[j];  // U = (B V) ./ transpose(D), images.jl:24
  return rect_apply_host(ctx, 0, k, V, U_out, inv.data(), true);  // with a shift: (C V) ./ ...
}

int rbl_set_rect_shift(rbl_ctx* ctx, const double* u, const double* v) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->rect) return fail(ctx, RBL_ERR_STATE, "rbl_set_rect_shift: no rectangular matrix");
  if ((u == nullptr) != (v == nullptr))
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_rect_shift: u and v must both be given or both be NULL");
  HIPC(hipSetDevice(ctx->device));
  if (!u) {  // clear: the operator is B^T B again
    HIPC(hipStreamSynchronize(ctx->stream));
    free_rect_shift(ctx);
    return RBL_OK;
  }
  const int64_t m = ctx->rect_m, n = ctx->n;
  for (int64_t i = 0; i < m; ++i)
    if (!std::isfinite(u[i])) return fail(ctx, RBL_ERR_INVALID, "rbl_set_rect_shift: u has a non-finite entry");
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return fail(ctx, RBL_ERR_INVALID, "rbl_set_rect_shift: v has a non-finite entry");
  HIPC(hipStreamSynchronize(ctx->stream));  // steps in flight still read the old vectors
  if (!ctx->d_shift_u) HIPC(ctx->d_shift_u.alloc(m));
  if (!ctx->d_shift_v) HIPC(ctx->d_shift_v.alloc(n));
  HIPC(hipMemcpy(ctx->d_shift_u, u, m * sizeof(double), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->d_shift_v, v, n * sizeof(double), hipMemcpyHostToDevice));
  ctx->rect_shift = true;
  return RBL_OK;
}

int rbl_get_rect_shift(rbl_ctx* ctx, double* u_out, double* v_out) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!ctx->rect || !ctx->rect_shift) return fail(ctx, RBL_ERR_STATE, "rbl_get_rect_shift: no shift set");
  HIPC(hipSetDevice(ctx->device));
  if (u_out) HIPC(hipMemcpy(u_out, ctx->d_shift_u, ctx->rect_m * sizeof(double), hipMemcpyDeviceToHost));
  if (v_out) HIPC(hipMemcpy(v_out, ctx->d_shift_v, ctx->n * sizeof(double), hipMemcpyDeviceToHost));
  return RBL_OK;
}

int rbl_apply_rect_shifted(rbl_ctx* ctx, int trans, int b, const double* X, double* Y) {
  if (!ctx || (trans != 0 && trans != 1) || b < 1 || b > RBL_MAX_BLOCK || !X || !Y)
    return fail(ctx, RBL_ERR_INVALID, "rbl_apply_rect_shifted: bad arguments");
  if (!ctx->rect) return fail(ctx, RBL_ERR_STATE, "rbl_apply_rect_shifted: no rectangular matrix");
  HIPC(hipSetDevice(ctx->device));
  return rect_apply_host(ctx, trans, b, X, Y, nullptr, true);
}

int rbl_matrix_info(rbl_ctx* ctx, int64_t* n, int64_t* row_begin, int64_t* row_end,
                    int64_t* nnz_local) {
  if (!ctx) return RBL_ERR_INVALID;
  if (n) *n = ctx->n;
  if (row_begin) *row_begin = ctx->r0;
  if (row_end) *row_end = ctx->r1;
  if (nnz_local) *nnz_local = ctx->nnz;
  return RBL_OK;
}

int rbl_row_ids(rbl_ctx* ctx, int64_t* ids) {
  if (!ctx || !ids) return RBL_ERR_INVALID;
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_row_ids: no matrix");
  for (int64_t i = 0; i < ctx->nloc; ++i)
    ids[i] = ctx->relabeled ? scatter_inv(ctx->relabel_perm, ctx->r0 + i) : ctx->r0 + i;
  return RBL_OK;
}

int rbl_get_matrix_csr(rbl_ctx* ctx, int64_t* rowptr, int32_t* colind, double* val) {
  if (ctx && ctx->csr_dropped)
    return fail(ctx, RBL_ERR_STATE, "rbl_get_matrix_csr: the CSR was released (RBL_OPT_KEEP_CSR = 0)");
  if (!ctx || !ctx->d_rowptr)
    return fail(ctx, RBL_ERR_STATE, ctx && ctx->dense  ? "dense matrix: no CSR"
                                    : ctx && ctx->kernop ? "kernel matrix: no CSR"
                                    : ctx && ctx->rect ? "rectangular matrix: use rbl_get_matrix_rect"
                                                       : "no matrix");
  HIPC(hipSetDevice(ctx->device));
  if (rowptr)
    HIPC(hipMemcpy(rowptr, ctx->d_rowptr, (ctx->nloc + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (colind && ctx->nnz)
    HIPC(hipMemcpy(colind, ctx->d_col, ctx->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (val && ctx->nnz)
    HIPC(hipMemcpy(val, ctx->d_val, ctx->nnz * sizeof(double), hipMemcpyDeviceToHost));
  return RBL_OK;
}

int rbl_spmm_kernel_for(rbl_ctx* ctx, int b) {
  if (!ctx || !has_matrix(ctx)) return RBL_ERR_INVALID;
  if (ctx->dense) return 4;
  if (ctx->rect) return 8;
  if (ctx->kernop) return RBL_SPMM_KERNEL_KERNOP;
  if (ctx->spmm_variant == 1) return 1;
  const int v = ctx->spmm_variant;
  const bool band = ctx->ntiles > 0 && ((b == 16 && ctx->band_ok16) || (b == 32 && ctx->band_ok32));
  const bool win = ctx->ntiles > 0 && ((b == 16 && ctx->window_ok16) || (b == 32 && ctx->window_ok32));
  const bool panel = b == 32 && ctx->panel_nblk > 0 && !ctx->csr_dropped && !ctx->ghost;
  if ((v == 0 || v == 4) && (b == 32 || b == 16) && (ctx->bt_ng == 5 || ctx->bt_ng == 9)) return 5;
  if ((v == 0 || v == 3 || v == 4) && band) return 3;
  if (((v == 0 && ctx->panel_auto) || v == 7) && panel) return 7;
  if ((v == 0 || v == 2 || v == 3) && win) return 2;
  if ((v == 0 || v == 5) && ctx->seg_ntasks > 0 && (b == 16 || b == 32)) return 6;
  return 1;
}

int rbl_matrix_format(rbl_ctx* ctx) {
  if (!ctx || !has_matrix(ctx)) return RBL_ERR_INVALID;
  if (ctx->dense) return 4;
  if (ctx->rect) return 5;
  if (ctx->kernop) return RBL_MATRIX_FORMAT_KERNOP;
  if (ctx->d_bth) return 3;
  if (ctx->d_btp_hdr) return 2;
  if (ctx->d_bt) return 1;
  return 0;
}

int rbl_apply(rbl_ctx* ctx, int b, const double* X, double* Y) {
  if (!ctx || b < 1 || b > RBL_MAX_BLOCK || !X || !Y) return fail(ctx, RBL_ERR_INVALID, "rbl_apply: bad arguments");
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_apply: no matrix");
  if (ctx->b != 0 && ctx->b != b && ctx->nranks > 1)
    return fail(ctx, RBL_ERR_STATE, "rbl_apply: b differs from the running Krylov block size");
  HIPC(hipSetDevice(ctx->device));
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  DevBuf<double> x, xr, y, ext;
  HIPC(x.alloc(nl * b));
  HIPC(xr.alloc(nl * b));
  HIPC(y.alloc((nl + kRowPad) * b));
  HIPC(hipMemcpyAsync(x, X, ctx->nloc * b * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  colmajor_to_rowmajor(x, ctx->nloc, b, xr, ctx->stream);
  const double* Qin = xr;
  int64_t off = 0;
  DevBuf<double> sendbuf;
  if (ctx->nranks > 1) {  // halo exchange through a private extended buffer
    const int64_t ext_rows = qext_rows(ctx, b);
    HIPC(ext.alloc(ext_rows * b));
    // rows between the received ranges stay finite (band-tile kernel multiplies them by 0)
    HIPC(hipMemsetAsync(ext, 0, ext_rows * b * sizeof(double), ctx->stream));
    if (use_ghost(ctx, b))
      HIPC(sendbuf.alloc(std::max<int64_t>(ctx->n_send, 1) * b));
    // the run's buffers and b step aside for the call's own, and come back whatever it returns
    size_t cap = (size_t)ext_rows * b;
    int bb = b;
    auto trade = [&] {
      std::swap(ctx->d_qext, ext);
      std::swap(ctx->qext_cap, cap);
      std::swap(ctx->d_sendbuf, sendbuf);
      std::swap(ctx->b, bb);
    };
    trade();
    const int st = halo_exchange(ctx, xr, &Qin, &off);
    trade();
    if (st < 0) return st;
  }
  {
    const int st = apply_A(ctx, Qin, off, b, y, nullptr, nullptr, nullptr);
    if (st < 0) return st;
  }
  HIPC(hipGetLastError());
  CHK(push_halo(ctx, xr, b, y));
  rowmajor_to_colmajor(y, ctx->nloc, b, x, ctx->stream);
  HIPC(hipMemcpyAsync(Y, x, ctx->nloc * b * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return RBL_OK;
}

int rbl_start(rbl_ctx* ctx, int b, int max_blocks, int basis_bits, const double* omega,
              uint64_t seed) {
  if (!ctx) return RBL_ERR_INVALID;
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_start: no matrix");
  if (b < 1 || b > RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "block size must be in [1," + std::to_string(RBL_MAX_BLOCK) + "]");
  if (max_blocks < 1) return fail(ctx, RBL_ERR_INVALID, "max_blocks must be >= 1");
  if (basis_bits != 64 && basis_bits != 32)
    return fail(ctx, RBL_ERR_INVALID, "basis_bits must be 64 or 32");
  if (ctx->rect && basis_bits != 64)
    return fail(ctx, RBL_ERR_INVALID, "rbl_start: a rectangular B (rbl_set_matrix_normal) needs the "
                                      "fp64 basis (basis_bits = 64)");
  if (ctx->kernop && basis_bits != 64)
    return fail(ctx, RBL_ERR_INVALID, "rbl_start: a kernel matrix (rbl_set_matrix_kernel) needs the fp64 "
                                      "basis (basis_bits = 64)");
  if (ctx->filt_deg > 0 && basis_bits != 64)
    return fail(ctx, RBL_ERR_INVALID, "rbl_start: a Chebyshev filter (rbl_set_filter) needs the fp64 "
                                      "basis (basis_bits = 64)");
  if (ctx->filt_deg > 0 && (ctx->rect || ctx->nranks > 1))
    return fail(ctx, RBL_ERR_INVALID, "rbl_start: a Chebyshev filter (rbl_set_filter) runs on one rank "
                                      "and a square A only");
  if (ctx->lr_r > 0 && basis_bits != 64)
    return fail(ctx, RBL_ERR_INVALID, "rbl_start: a low-rank update (rbl_set_lowrank) needs the fp64 "
                                      "basis (basis_bits = 64)");
  if (has_series(ctx) && basis_bits != 64)
    return fail(ctx, RBL_ERR_INVALID, "rbl_start: a Chebyshev series (rbl_set_filter_series) needs the "
                                      "fp64 basis (basis_bits = 64)");
  if (has_series(ctx) && (ctx->rect || ctx->nranks > 1))
    return fail(ctx, RBL_ERR_INVALID, "rbl_start: a Chebyshev series (rbl_set_filter_series) runs on "
                                      "one rank and a square A only");
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  // a repeated run with the same shape reuses the HBM plan (allocating ~100 GB of basis
  // per run costs more than the run itself at n = 1e7)
  // device slots of the basis (RBL_OPT_DEVICE_BLOCKS; RBL_gpu.jl:95-104 gpu_buffer_size)
  int dev_slots = max_blocks + 1;
  // the shape of the current plan matches: the automatic plan (G = -1) keeps its slot count
  // instead of re-deriving it from the free memory its own buffers now occupy — re-planning
  // frees and re-allocates the basis and unpins / re-pins every host spill slot (C5: ~40 s per
  // run on the host, hipHostMalloc / hipHostFree of ~80 GB)
  const bool same_shape = (ctx->d_basis || ctx->d_basis32) && ctx->b == b &&
                          ctx->max_blocks == max_blocks && ctx->slot == ctx->nloc * b &&
                          ctx->basis_bits == basis_bits;
  const int cur_slots = ctx->resident == INT32_MAX ? ctx->max_blocks + 1 : ctx->resident + 2;
  if (ctx->dev_blocks_opt < 0 && same_shape && ctx->auto_planned) {
    dev_slots = cur_slots;
  } else if (ctx->dev_blocks_opt != 0) {
    int g = ctx->dev_blocks_opt;
    if (g < 0) {
      size_t fr = 0, tot = 0;
      HIPC(hipMemGetInfo(&fr, &tot));
      // the basis is typed FLOAT (RBL_gpu.jl:59-81, 95-104): slots of n_local x b x s bytes
      const double blk64 = (double)std::max<int64_t>(ctx->nloc, 1) * b * 8.0;
      const double blk = blk64 * (basis_bits == 64 ? 1.0 : 0.5);
      // what the run needs beside the basis: U, T, the halo copy, staging, the fp64 working
      // block of the fp32 path, ~slab; a run already planned frees its buffers first
      const double mine = ctx->d_basis ? (double)(ctx->resident == INT32_MAX ? ctx->max_blocks + 1 : ctx->resident + 2) * blk64
                        : ctx->d_basis32 ? (double)(ctx->resident == INT32_MAX ? ctx->max_blocks + 1 : ctx->resident + 2) * blk64 * 0.5
                        : 0.0;
      // (the fp32 shadow is freed with the plan and never weighs on the slot count)
      const double mine_all = mine + (double)ctx->shadow_bytes;
      // U, T (+ the halo buffer on several ranks; + the fp32 path's fp64 Q_i, and Q_{i-1}
      // when the SpMM cannot read fp32), one staging block, the Gram slab
      const double work = 2.0 + (ctx->nranks > 1 ? 1.0 : 0.0) +
                          (basis_bits == 32 ? 1.0 + (direct32_ok(ctx, b) ? 0.0 : 1.0) : 0.0);
      const double other = work * blk64 + blk + 8.0 * (double)gram_slab_elems(ctx, b, max_blocks, basis_bits);
      g = (int)std::max(3.0, std::floor((0.8 * ((double)fr + mine_all) - other) / blk));
    }
    dev_slots = std::min(dev_slots, std::max(3, g));
  }
  const bool reuse = same_shape && cur_slots == dev_slots;
  ctx->plan_all_resident = ctx->dev_blocks_opt == 0;  // an option: the same on every rank
  ctx->nlock = 0;  // a new problem: no locked vectors
  ctx->arrow_kb = 0;
  ctx->cloc_step = 0;
  ctx->shadow_valid = 0;
  ctx->step_flags.clear();
  // the allocations below fail alone on one rank (its HBM): every rank then learns of it before
  // the collectives of the start, and all return the error, instead of the peers waiting in the
  // halo exchange for a rank that has left
  const int alloc_st = [&]() -> int {
  if (reuse) {
    ctx->nblocks = 0;
    if (ctx->cstream) HIPC(hipStreamSynchronize(ctx->cstream));
    ctx->d2h_pending[0] = ctx->d2h_pending[1] = false;
    HIPC(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), ctx->stream));
  } else {
  free_run(ctx);
  ctx->b = b;
  ctx->max_blocks = max_blocks;
  ctx->slot = ctx->nloc * b;
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  ctx->basis_bits = basis_bits;
  ctx->auto_planned = ctx->dev_blocks_opt < 0;
  if (basis_bits == 64) {
    HIPC(ctx->d_basis.alloc((size_t)dev_slots * nl * b));
    if (dev_slots < max_blocks + 1) {  // host spill: pinned slots for blocks resident..max_blocks
      ctx->resident = dev_slots - 2;
      // non-coherent pinned pages: the DMA engines stream them at PCIe rate both ways
      ctx->h_spill = std::vector<PinBuf<char>>(max_blocks + 1 - ctx->resident);
      HIPC(ctx->d_stage.alloc((size_t)nl * b));
      CHK(ensure_spill_stream(ctx));
    }
  } else {
    // + kRowPad32 zeroed pad rows, and every slot zeroed once: the fp32 Gram kernel's shifted
    // chunks may read rows past a tiny slice (reorth32.hip), which must be finite
    const size_t len32 = ((size_t)dev_slots * nl + kRowPad32) * b;
    HIPC(ctx->d_basis32.alloc(len32));
    HIPC(hipMemsetAsync(ctx->d_basis32, 0, len32 * sizeof(float), ctx->stream));
    if (dev_slots < max_blocks + 1) {  // host spill of the FLOAT basis (RBL_gpu.jl:59-81)
      ctx->resident = dev_slots - 2;
      ctx->h_spill = std::vector<PinBuf<char>>(max_blocks + 1 - ctx->resident);
      // + kRowPad32 zero rows like the slots (the Gram's shifted chunks)
      HIPC(ctx->d_stage32.alloc(((size_t)nl + kRowPad32) * b));
      HIPC(hipMemsetAsync(ctx->d_stage32, 0, ((size_t)nl + kRowPad32) * b * sizeof(float), ctx->stream));
      CHK(ensure_spill_stream(ctx));
    }
    HIPC(ctx->d_Qi64.alloc((nl + kRowPad) * b));
    // the widened Q_{i-1}: only when the SpMM cannot read the fp32 blocks directly
    if (!direct32_ok(ctx, b)) HIPC(ctx->d_Qm64.alloc((nl + kRowPad) * b));
  }
  HIPC(ctx->d_U.alloc((nl + kRowPad) * b));
  ctx->T_cols = b;
  HIPC(ctx->d_T.alloc(nl * b));
  if (ctx->nranks > 1) {
    CHK(ensure_qext(ctx, b, ctx->stream));
    if (ctx->ghost)
      HIPC(ctx->d_sendbuf.alloc(std::max<int64_t>(ctx->n_send, 1) * b));
  }
  const size_t slab = gram_slab_elems(ctx, b, max_blocks, basis_bits);
  ctx->slab_elems = slab;
  HIPC(ctx->d_slab.alloc(slab));
  ctx->C_elems = (size_t)std::max(1, max_blocks) * b * 2 * b;
  HIPC(ctx->d_C.alloc(ctx->C_elems));
  if (b == 32) HIPC(ctx->d_C16.alloc((size_t)tsmm44x32_cpieces(std::max(1, max_blocks) * b)));  // (k_tsmm44x32's image of d_C)
  HIPC(ctx->d_small.alloc((size_t)S_NSMALL * b * b));
  HIPC(hipMemset(ctx->d_small, 0, (size_t)S_NSMALL * b * b * sizeof(double)));  // (S_CX is summed before it is first written)
  HIPC(ctx->d_flags.alloc(6));
  HIPC(hipMemset(ctx->d_flags, 0, 6 * sizeof(int)));
  if (!ctx->d_upd32) {  // kept across runs: its counters are rbl_path_stats entries
    HIPC(ctx->d_upd32.alloc(6));
    HIPC(hipMemset(ctx->d_upd32, 0, 6 * sizeof(int)));
    HIPC(ctx->d_upd32_g.alloc(kUpd32Log));
    HIPC(hipMemset(ctx->d_upd32_g, 0, kUpd32Log * sizeof(double)));
  }
  {
#ifdef RBL_VARIANTS
    const char* e = std::getenv("RBL_STASH_COPY");  // A/B: 1 = device record + D2H copy
    ctx->stash_direct = !(e && std::atoi(e) == 1);
#else
    ctx->stash_direct = true;
#endif
    const unsigned hf = ctx->stash_direct ? (hipHostMallocMapped | hipHostMallocCoherent) : hipHostMallocDefault;
    HIPC(ctx->h_pin.alloc(stash_rec(b), hf));
    HIPC(ctx->h_hist.alloc((size_t)(max_blocks + 2) * stash_rec(b), hf));
    if ((size_t)ctx->nloc * b * sizeof(double) >= 4 * kD2HPiece && !d2h_direct()) {
      CHK(ensure_d2h_slots(ctx));
      CHK(ensure_ritz_stream(ctx));
    }
    if (ctx->stash_direct) {
      HIPC(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->dv_pin), ctx->h_pin, 0));
      HIPC(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->dv_hist), ctx->h_hist, 0));
    } else {
      HIPC(ctx->d_stash.alloc(stash_rec(b)));
    }
  }
  // RBL_OPT_UPD32_SHADOW, after everything the run needs: only where the fp32 update can run
  // (fp64 basis, b = 32, RBL_OPT_UPD32 on, every block in HBM) and only into memory the fit rule
  // leaves over.  Kept with the plan (a reused plan allocates nothing), freed by free_run.  A rank
  // that goes without takes the fp64-basis loads: no collective and no bit differs.
  if (ctx->shadow_opt && ctx->upd32 != 0 && basis_bits == 64 && b == 32 && !spilled(ctx) &&
      max_blocks >= 3 && ctx->nloc > 0) {
    const int64_t sslot = tsmm44x32_shadow_slot(ctx->nloc);
    const size_t need = (size_t)(max_blocks - 2) * (size_t)sslot * sizeof(float);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && rbl_plan_shadow_fits(fr, tot, need)) {
      if (ctx->d_shadow.alloc((size_t)(max_blocks - 2) * (size_t)sslot) == hipSuccess) {
        ctx->shadow_slot = sslot;
        ctx->shadow_bytes = need;
      } else {
        (void)hipGetLastError();  // the run goes on without the shadow
      }
    }
  }
  }
  // the push/pull split's partial-row buffers (sized by the matrix held, so also on a reused
  // plan): allocated here, inside the vote, not lazily in the first push exchange — a rank
  // failing there would leave its peers waiting in that exchange
  if (ctx->push && ctx->nranks > 1 && use_ghost(ctx, b)) {  // push_on() once this b exchanges
    const char* inj = std::getenv("RBL_FAULT_PUSH_ALLOC");  // fault injection for the vote's test
    if (inj && *inj && std::atoi(inj) == ctx->rank)
      return fail(ctx, RBL_ERR_OOM, "rbl_start: push buffers (injected by RBL_FAULT_PUSH_ALLOC)");
    CHK(ensure_push(ctx, b));
  }
  if (has_filter(ctx)) CHK(ensure_filter_bufs(ctx, b));
  return RBL_OK;
  }();
  if (ctx->nranks > 1) {
    const int64_t mine = alloc_st;
    std::vector<int64_t> all(ctx->nranks);
    COMMC(ctx->comm->allgather_host(&mine, all.data(), 1, ctx->stream, &ctx->err));
    int bad = -1;
    for (int q = 0; q < ctx->nranks && bad < 0; ++q)
      if (all[q] != RBL_OK) bad = q;
    if (bad >= 0) {
      (void)hipGetLastError();  // the failed hipMalloc's error must not surface in a later check
      free_run(ctx);  // (a later start re-plans from scratch)
      if (alloc_st != RBL_OK) return alloc_st;
      return fail(ctx, (int)all[bad], "rbl_start: rank " + std::to_string(bad) +
                                          " could not allocate its run buffers");
    }
  } else if (alloc_st != RBL_OK) {
    (void)hipGetLastError();
    return alloc_st;
  }

  // Omega (row-major) in d_T
  if (omega) {
    double* d_tmp = ctx->d_U;  // free until A * Omega
    HIPC(hipMemcpyAsync(d_tmp, omega, ctx->nloc * b * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
    colmajor_to_rowmajor(d_tmp, ctx->nloc, b, ctx->d_T, ctx->stream);
  } else {
    randn_block(ctx->d_T, ctx->nloc, b, ctx->r0, seed, ctx->stream,
                ctx->relabeled ? &ctx->relabel_perm : nullptr);
  }
  // Q_1 = qr(A * Omega).Q   (RBL_gpu.jl:213-214)
  const double* Qin = nullptr;
  int64_t off = 0;
  CHK(halo_exchange(ctx, ctx->d_T, &Qin, &off));
  {
    StageScope t(ctx, RBL_STAGE_AQ);
    if (has_filter(ctx))  // Q_1 = qr(p(A) Omega).Q
      CHK(filter_apply(ctx, ctx->d_T, b, ctx->d_U, ctx->d_filt));
    else
      CHK(apply_A(ctx, Qin, off, b, ctx->d_U, nullptr, nullptr, nullptr));
    HIPC(hipGetLastError());
  }
  CHK(push_halo(ctx, ctx->d_T, b, ctx->d_U));
  if (basis_bits == 64) {
    CHK(tsqr(ctx, ctx->d_U, slotp(ctx, 0)));
  } else {  // step 1 multiplies the unrounded fp64 Q_1 (RBL_gpu.jl:142, 152); the basis holds fp32
    CHK(tsqr(ctx, ctx->d_U, ctx->d_Qi64));
    cvt_f64_to_f32(ctx->d_Qi64, slotp32(ctx, 0), ctx->nloc * b, ctx->stream);
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  int flags[4];
  HIPC(hipMemcpy(flags, ctx->d_flags, sizeof(flags), hipMemcpyDeviceToHost));
  if (flags[2]) return fail(ctx, RBL_ERR_NUMERIC, "QR breakdown in rbl_start");
  ctx->nblocks = 1;
  ctx->fetched = 1;
  return RBL_OK;
}

namespace {
int step_impl(rbl_ctx* ctx, int i, int part_reorth, double* A_out, double* B_out, bool async);
}
int rbl_step(rbl_ctx* ctx, int i, int part_reorth, double* A_out, double* B_out) {
  if (ctx && ctx->fetched < ctx->nblocks)
    return fail(ctx, RBL_ERR_STATE, "rbl_step: rbl_fetch the asynchronous steps first");
  const int rc = step_impl(ctx, i, part_reorth, A_out, B_out, false);
  if (ctx && rc >= 0) ctx->fetched = ctx->nblocks;
  return rc;
}
int rbl_step_async(rbl_ctx* ctx, int i, int part_reorth) {
  return step_impl(ctx, i, part_reorth, nullptr, nullptr, true);
}
int rbl_fetch(rbl_ctx* ctx, int i0, int i1, double* A_out, double* B_out, int* status_out) {
  if (!ctx) return RBL_ERR_INVALID;
  if (i0 != ctx->fetched || i1 < i0 || i1 > ctx->nblocks)
    return fail(ctx, RBL_ERR_INVALID, "rbl_fetch: [i0, i1) must start at the first unfetched step");
  HIPC(hipSetDevice(ctx->device));
  // steps enqueued after i1 - 1 (speculatively, while the host works on the T band) keep running
  const int last = i1 - 1;
  if (last >= 1 && last < (int)ctx->step_ev.size() && ctx->step_ev[last])
    HIPC(hipEventSynchronize(ctx->step_ev[last]));
  else
    HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  const int b = ctx->b;
  int rc = RBL_OK;
  for (int j = i0; j < i1; ++j) {
    const double* h = ctx->h_hist + (size_t)j * stash_rec(b);
    const int* fl = reinterpret_cast<const int*>(h + 2 * b * b);
    double* A = A_out ? A_out + (size_t)(j - i0) * b * b : nullptr;
    double* B = B_out ? B_out + (size_t)(j - i0) * b * b : nullptr;
    for (int r = 0; r < b; ++r)
      for (int c = 0; c < b; ++c) {
        if (A) A[c * b + r] = h[r * b + c];
        if (B) B[c * b + r] = h[b * b + r * b + c];
      }
    const int st = fl[2] ? RBL_ERR_NUMERIC : fl[3] ? RBL_WARN_QR_SHIFTED : RBL_OK;
    if (status_out) status_out[j - i0] = st;
    if (st == RBL_ERR_NUMERIC && rc >= 0) rc = fail(ctx, RBL_ERR_NUMERIC, "QR breakdown (shifted CholQR failed)");
  }
  ctx->fetched = i1;
  return rc;
}
namespace {
int step_impl(rbl_ctx* ctx, int i, int part_reorth, double* A_out, double* B_out, bool async) {
  if (!ctx) return RBL_ERR_INVALID;
  if ((!ctx->d_basis && !ctx->d_basis32) || ctx->nblocks < 1) return fail(ctx, RBL_ERR_STATE, "rbl_step before rbl_start");
  if (i != ctx->nblocks) return fail(ctx, RBL_ERR_STATE, "rbl_step: i must equal the current block count");
  if (i > ctx->max_blocks) return fail(ctx, RBL_ERR_STATE, "rbl_step: basis full (max_blocks)");
  HIPC(hipSetDevice(ctx->device));
  const int b = ctx->b;
  const bool f32 = ctx->basis_bits == 32;
  if (!ctx->flags_clean) HIPC(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), ctx->stream));
  ctx->flags_clean = false;  // until this step's k_stash has run
  if (f32 && (part_reorth & 2))
    return fail(ctx, RBL_ERR_INVALID, "rbl_step: locked-vector reorth needs the fp64 basis");
  // fp32 basis with the band-tile SpMM: A Q_i (after an fp32 halo exchange) and the 3-term
  // update read the fp32 blocks and widen them on load — bit for bit the widened copies
  // (RBL_gpu.jl:173-174), without the two conversion passes.  Step 1 multiplies the unrounded
  // fp64 Q_1 of rbl_start.
  const bool direct32 = f32 && i >= 2 && direct32_ok(ctx, b);
  if (f32 && !direct32) CHK(ensure_qm64(ctx));
  double* Qi = f32 ? ctx->d_Qi64 : slotp(ctx, i - 1);
  double* Qm = i >= 2 ? (f32 ? ctx->d_Qm64 : slotp(ctx, i - 2)) : nullptr;
  float* Qi32 = f32 ? slotp32(ctx, i - 1) : nullptr;
  float* Qm32 = f32 && i >= 2 ? slotp32(ctx, i - 2) : nullptr;
  if (f32) {
    // FLOAT = Float32: partial and local reorth on the fp32 blocks, then the
    // current / previous block widened to fp64 (RBL_gpu.jl:164-174)
    if ((part_reorth & 1) && i >= 3) {
      StageScope t(ctx, RBL_STAGE_PART_REORTH);
      const int nW = i - 2;
      const int nres = std::min(nW, ctx->resident);  // HBM-resident part of W
      if (ctx->reorth_order == 0) {
        CHK(gram32(ctx, slotp32(ctx, 0), nres, Qi32, Qm32, 2, ctx->d_C));
        CHK(upd32(ctx, slotp32(ctx, 0), nres, ctx->d_C, 2 * b, Qi32, Qm32, 2));
      } else {
        for (int j = 0; j < nres; ++j) {
          CHK(gram32(ctx, slotp32(ctx, j), 1, Qi32, Qm32, 2, ctx->d_C));
          CHK(upd32(ctx, slotp32(ctx, j), 1, ctx->d_C, 2 * b, Qi32, Qm32, 2));
        }
      }
      // spilled fp32 blocks streamed back in ascending j (RBL_gpu.jl:65-68 with FLOAT)
      for (int j = nres; j < nW; ++j) {
        int st = 0;
        const float* Wj = block_dev32(ctx, j, i, &st);
        if (st) return fail(ctx, st, "partial reorth: H2D of a spilled block failed");
        CHK(gram32(ctx, Wj, 1, Qi32, Qm32, 2, ctx->d_C));
        CHK(upd32(ctx, Wj, 1, ctx->d_C, 2 * b, Qi32, Qm32, 2));
      }
    }
    // host spill: block i-2 is final (RBL_gpu.jl:76) — copied out on the side stream; the
    // QR of this step, which rewrites its working slot, waits for the copy
    if (spilled(ctx) && i >= 2 && i - 2 >= ctx->resident) {
      HIPC(hipEventRecord(ctx->ev_fin, ctx->stream));
      HIPC(hipStreamWaitEvent(ctx->cstream, ctx->ev_fin, 0));
      CHK(spill_slot(ctx, i - 2, sizeof(float)));
      HIPC(hipMemcpyAsync(ctx->h_spill[i - 2 - ctx->resident], Qm32,
                          ctx->slot * sizeof(float), hipMemcpyDeviceToHost, ctx->cstream));
      HIPC(hipEventRecord(ctx->ev_d2h[i & 1], ctx->cstream));
      ctx->d2h_pending[i & 1] = true;
    }
    if (i >= 2) {
      StageScope t(ctx, RBL_STAGE_LOC_REORTH);
      CHK(gram32(ctx, Qm32, 1, Qi32, nullptr, 1, ctx->d_C));
      CHK(upd32(ctx, Qm32, 1, ctx->d_C, b, Qi32, nullptr, 1));
      if (!direct32) {
        cvt_f32_to_f64(Qi32, ctx->d_Qi64, ctx->nloc * b, ctx->stream);
        cvt_f32_to_f64(Qm32, ctx->d_Qm64, ctx->nloc * b, ctx->stream);
      }
      HIPC(hipGetLastError());
    }
  }

  // partial reorth of Q_i and Q_{i-1} against Q_1..Q_{i-2}   (RBL_gpu.jl:164-166, 59-81),
  // preceded (flag bit 1, restarted variants) by the reorth against the locked vectors
  if (!f32) CHK(reorth_pair(ctx, i, part_reorth));
  // host spill: block i-2 is final now (the hybrid buffer's `copyto!(Q[i-1], Qg1)`,
  // RBL_gpu.jl:76): copy it out on the side stream while the step goes on; its working slot
  // is rewritten by this step's QR, which waits for the copy
  if (!f32 && spilled(ctx) && i >= 2 && i - 2 >= ctx->resident) {
    HIPC(hipEventRecord(ctx->ev_fin, ctx->stream));
    HIPC(hipStreamWaitEvent(ctx->cstream, ctx->ev_fin, 0));
    CHK(spill_slot(ctx, i - 2, sizeof(double)));
    HIPC(hipMemcpyAsync(ctx->h_spill[i - 2 - ctx->resident], slotp(ctx, i - 2),
                        ctx->slot * sizeof(double), hipMemcpyDeviceToHost, ctx->cstream));
    HIPC(hipEventRecord(ctx->ev_d2h[i & 1], ctx->cstream));
    ctx->d2h_pending[i & 1] = true;
  }
  // local reorth: Q_i -= Q_{i-1} (Q_{i-1}^T Q_i), one projection (RBL_gpu.jl:83-93, P1)
  const bool fused = rowgram_ok(b);
  // Q_i / Q_{i-1} change before the local reorth of this step iff it runs a partial or
  // locked-vector reorth; otherwise the Gram formed by the previous step's QR is current
  auto modifies = [&](int step, int flags) {
    return ((flags & 1) && step >= 3) || ((flags & 2) && ctx->nlock > 0);
  };
  if ((int)ctx->step_flags.size() <= i) ctx->step_flags.resize(i + 1, 0);
  ctx->step_flags[i] = part_reorth;
  // fuse bit 2: the update itself rides on the SpMM below, which stages Q_i's rows corrected
  // (fp64 basis, band tiles at b = 32; no collective depends on the choice)
  // (not with a Chebyshev filter: the staging fusion assumes U = A Q_i from one SpMM)
  const bool filt = has_filter(ctx);
  // the arrow step after a thick restart (rbl_thick_restart): Q_i = Q_{m+1} couples to every kept
  // block, U = Op Q_i - [Y_1 .. Y_kb] W^T; the operator runs without the 3-term epilogue, the local
  // reorth on its own pass (the staging fusion assumes the plain 3-term shape) and A_i comes from
  // the Gram of the final U
  const bool arrow = ctx->arrow_kb > 0 && i == ctx->arrow_kb + 1;
  if (arrow && (f32 || spilled(ctx) || ctx->nranks > 1))
    return fail(ctx, RBL_ERR_STATE, "rbl_step: the arrow step needs one rank and an HBM-resident fp64 basis");
  auto arrow_update = [&]() -> int {  // U -= [Y_1 .. Y_kb] W^T, one tsmm over the kept run
    PanelRun Y;
    Y.base = slotp(ctx, 0);
    Y.stride = ctx->slot;
    Y.count = ctx->arrow_kb;
    Y.w = b;
    return tsmm_checked(ctx, Y, ctx->d_arrow_W, b, pan1(ctx->d_U, b), -1.0, 1.0, nullptr);
  };
  const bool lfuse = !f32 && i >= 2 && (ctx->fuse & 4) && fused && !ctx->dense && ctx->nloc > 0 &&
                     !filt && !arrow && rbl_spmm_kernel_for(ctx, b) == 5 && spmm_bt_locfix_ok(csr(ctx), b);
  const double* Cloc = nullptr;
  int64_t lf_lo = 0, lf_hi = ctx->nloc;
  if (!f32 && i >= 2) {
    StageScope t(ctx, RBL_STAGE_LOC_REORTH);
    const bool have = ctx->cloc_step == i && (ctx->cloc_final || !modifies(i, part_reorth));
    const double* C = have ? smallp(ctx, S_CLOC) : ctx->d_C;
    if (!have) {
      CHK(gram(ctx, run1(Qm, b), pan1(Qi, b), ctx->d_C, nullptr));
      ctx->path_stats[RBL_PATH_LOC_GRAM] += 1;
    } else if (ctx->cloc_src == 1) {
      ctx->path_stats[RBL_PATH_CLOC_3TERM] += 1;
    } else if (ctx->cloc_src == 2) {
      ctx->path_stats[RBL_PATH_CLOC_REORTH] += 1;
    }
    if (lfuse) {
      Cloc = C;
      if (ctx->nranks > 1) {  // the rows the neighbours receive: corrected before the exchange
        const int64_t H = spmm_bt_halfwidth(csr(ctx));
        lf_lo = std::min<int64_t>(H, ctx->nloc);
        lf_hi = std::max<int64_t>(lf_lo, ctx->nloc - H);
        spmm_bt_locfix_edges(csr(ctx), Qi, Qm, C, 0, lf_lo, lf_hi, ctx->nloc, ctx->stream);
        HIPC(hipGetLastError());
        ctx->path_stats[RBL_PATH_LOCFIX_EDGES] += 1;
      }
    } else if (fused) {
      CHK(rowop(ctx, Qm, C, Qi, -1.0, 1.0, nullptr, nullptr));
      ctx->path_stats[RBL_PATH_LOC_SEPARATE] += 1;
    } else {
      CHK(tsmm_checked(ctx, run1(Qm, b), C, b, pan1(Qi, b), -1.0, 1.0, nullptr));
      ctx->path_stats[RBL_PATH_LOC_SEPARATE] += 1;
    }
  }
  ctx->cloc_step = 0;
  ctx->cloc_final = false;
  // U = A Q_i - Q_{i-1} B_i^T   (RBL_gpu.jl:176-177)
  int ai_parts = 0;
  bool pushed = false;  // the push/pull split's partials sent on the side stream
  if (filt) {
    // U = p(A) Q_i - Q_{i-1} B_i^T (one rank, fp64 basis): the recurrence reads Q_i and leaves
    // it and Q_{i-1} as they are; no fused route of the plain step applies (no local-reorth
    // staging, no A_i partials, no split source), A_i = Q_i^T U comes from the Gram below
    if (f32 || ctx->nranks > 1 || ctx->rect)
      return fail(ctx, RBL_ERR_INVALID, "rbl_step: a Chebyshev filter needs one rank, a square A and "
                                        "the fp64 basis");
    CHK(ensure_filter_bufs(ctx, b));
    StageScope t(ctx, RBL_STAGE_AQ);
    CHK(filter_apply(ctx, Qi, b, ctx->d_U, ctx->d_filt));
    if (arrow) {
      CHK(arrow_update());
    } else if (i >= 2) {
      transpose_small(smallp(ctx, S_BPREV), smallp(ctx, S_BT), b, ctx->stream);
      CHK(tsmm_checked(ctx, run1(Qm, b), smallp(ctx, S_BT), b, pan1(ctx->d_U, b), -1.0, 1.0, nullptr));
    }
    HIPC(hipGetLastError());
  } else {
    const double* Qin = nullptr;
    const float* Qin32 = nullptr;
    int64_t off = 0;
    // several ranks with the band-tile kernel: the halo buffer takes only the neighbours'
    // rows; the kernel reads the own rows from the block (no per-step local copy)
    const int kid = rbl_spmm_kernel_for(ctx, b);
    const bool seg_split = !direct32 && kid == 6 && ctx->seg_split;
    const bool split = ctx->nranks > 1 && !ctx->dense &&
                       (direct32 || kid == 5 || seg_split) && ctx->split_halo;
    // unbanded A on several ranks (the halo is most of Q_i): the exchange runs on a side
    // stream while the SpMM's own-column tier runs; the halo tier waits for it
    // (RBL_OPT_HALO_OVERLAP; the same sums in the same order either way)
    const bool overlap = split && seg_split && ctx->halo_overlap;
    hipEvent_t halo_ev = nullptr;
    if (overlap) {
      if (!ctx->hstream) {
        HIPC(hipStreamCreateWithFlags(&ctx->hstream, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&ctx->ev_qready, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&ctx->ev_halo, hipEventDisableTiming));
      }
      HIPC(hipEventRecord(ctx->ev_qready, ctx->stream));  // Q_i final (local reorth done)
      HIPC(hipStreamWaitEvent(ctx->hstream, ctx->ev_qready, 0));
      CHK(halo_exchange(ctx, Qi, &Qin, &off, false, ctx->hstream));
      HIPC(hipEventRecord(ctx->ev_halo, ctx->hstream));
      halo_ev = ctx->ev_halo;
      if (push_on(ctx)) {  // the partials go out behind the pulled rows, before the SpMM
        if (!ctx->ev_push_ready) {
          HIPC(hipEventCreateWithFlags(&ctx->ev_push_ready, hipEventDisableTiming));
          HIPC(hipEventCreateWithFlags(&ctx->ev_push_done, hipEventDisableTiming));
        }
        CHK(push_products(ctx, Qi, b, ctx->stream));
        HIPC(hipEventRecord(ctx->ev_push_ready, ctx->stream));
        HIPC(hipStreamWaitEvent(ctx->hstream, ctx->ev_push_ready, 0));
        CHK(push_exchange(ctx, b, ctx->hstream));
        HIPC(hipEventRecord(ctx->ev_push_done, ctx->hstream));
        pushed = true;
      }
    } else if (direct32) {
      CHK(halo_exchange32(ctx, Qi32, &Qin32, &off, !split));
    } else {
      CHK(halo_exchange(ctx, Qi, &Qin, &off, !split));
    }
    StageScope t(ctx, RBL_STAGE_AQ);
    // the band kernel can also form the partials of A_i = Q_i^T U while U is in registers
    if (direct32) {
      CsrDev A = csr(ctx);
      if (split) {
        A.qloc = Qi32;
        A.loc_lo = ctx->r0;
        A.loc_hi = ctx->r0 + ctx->nloc;
      }
      if (!spmm_bt(A, nullptr, off, b, ctx->d_U, nullptr, smallp(ctx, S_BPREV), ctx->stream,
                   ctx->d_slab, &ai_parts, Qin32, Qm32))
        return fail(ctx, RBL_ERR_INVALID, "internal: fp32 band-tile SpMM not applicable");
    } else {
      ai_parts = apply_A(ctx, Qin, off, b, ctx->d_U, arrow ? nullptr : Qm,
                         i >= 2 && !arrow ? smallp(ctx, S_BPREV) : nullptr, arrow ? nullptr : ctx->d_slab,
                         split ? Qi : nullptr, Cloc, Qi, lf_lo, lf_hi, halo_ev);
      if (arrow && ai_parts >= 0) {
        ai_parts = 0;
        CHK(arrow_update());
      }
    }
    if (ai_parts < 0) return ai_parts;
    HIPC(hipGetLastError());
    // the main stream's next collective must follow the side stream's exchange on every rank,
    // also where the SpMM never waited for it (a rank without rows returns from apply_A early)
    if (halo_ev) HIPC(hipStreamWaitEvent(ctx->stream, halo_ev, 0));
  }
  if (arrow) ctx->arrow_kb = 0;
  // the push/pull split: the received partials into U (A_i is formed after this, from all of U)
  if (pushed) {
    HIPC(hipStreamWaitEvent(ctx->stream, ctx->ev_push_done, 0));
    CHK(push_finish(ctx, ctx->d_U, b, ctx->stream));
  } else if (!direct32 && ai_parts == 0) {
    CHK(push_halo(ctx, Qi, b, ctx->d_U));
  }
  // A_i = Q_i^T U ; U -= Q_i A_i   (RBL_gpu.jl:178-179); fused: the update pass also forms
  // U^T U, CholQR's first Gram
  // RBL_OPT_CLOC_DERIVE: the update pass also forms M = Q_i^T U', which the QR below turns into
  // the next step's local-reorth coefficient (on every step: no guess of that step's schedule)
  const bool cloc_m = cloc_derive_on(ctx) && !filt && !arrow && i + 1 <= ctx->max_blocks;
  {
    StageScope t(ctx, RBL_STAGE_3TERM);
    if (ai_parts > 0) {
      reduce_slab(ctx->d_slab, ai_parts, (int64_t)b * b, smallp(ctx, S_AI), nullptr, ctx->stream);
      HIPC(hipGetLastError());
      CHK(allreduce(ctx, smallp(ctx, S_AI), (size_t)b * b));
    } else {
      CHK(gram(ctx, run1(Qi, b), pan1(ctx->d_U, b), smallp(ctx, S_AI), nullptr));
    }
    if (cloc_m)
      CHK(rowop_3term_cloc(ctx, Qi, ctx->d_U));
    else if (fused)
      CHK(rowop(ctx, Qi, smallp(ctx, S_AI), ctx->d_U, -1.0, 1.0, smallp(ctx, S_G), nullptr,
                direct32 ? Qi32 : nullptr));
    else
      CHK(tsmm_checked(ctx, run1(Qi, b), smallp(ctx, S_AI), b, pan1(ctx->d_U, b), -1.0, 1.0, nullptr));
  }
  // Q_{i+1} B_{i+1} = qr(U)   (RBL_gpu.jl:180-184)
  if (ctx->d2h_pending[i & 1]) {  // the working slot's previous block is on the host
    StageScope t(ctx, RBL_STAGE_SPILL_WAIT);  // the stream stalls here until that copy is done
    HIPC(hipStreamWaitEvent(ctx->stream, ctx->ev_d2h[i & 1], 0));
    ctx->d2h_pending[i & 1] = false;
  }
  if (!f32) {
    // the next step's local-reorth Gram Q_i^T Q_{i+1} rides on this QR when that step is
    // expected to run no partial reorth (the schedule repeats with period 2 in RBL_gpu.jl:164,
    // so step i + 1 is guessed from step i - 1; a wrong guess costs one pass, never bits)
    const int guess = i >= 2 ? ctx->step_flags[i - 1] : 0;
    const bool zfuse = !cloc_m && fused && (ctx->fuse & 3) == 3 && !modifies(i + 1, guess) &&
                       i + 1 <= ctx->max_blocks;
    CHK(tsqr(ctx, ctx->d_U, slotp(ctx, i), fused, nullptr, zfuse || cloc_m ? Qi : nullptr, cloc_m));
    if (zfuse || cloc_m) {
      ctx->cloc_step = i + 1;
      ctx->cloc_final = false;
      ctx->cloc_src = cloc_m ? 1 : 0;
    }
  } else {  // Qg = FLOAT(Qg_d) (RBL_gpu.jl:182): the new block enters the basis rounded to fp32
    CHK(tsqr(ctx, ctx->d_U, ctx->d_Qi64, fused, slotp32(ctx, i)));
  }
  // B_prev = R_tot, and A_i, R_tot, flags as one record: written to the host by k_stash itself
  // (or one D2H copy of the device record, RBL_STASH_COPY=1)
  const size_t rec = stash_rec(b);
  double* rec_dev = !ctx->stash_direct ? ctx->d_stash
                    : async            ? ctx->dv_hist + (size_t)i * rec
                                       : ctx->dv_pin;
  stash_step(smallp(ctx, S_AI), smallp(ctx, S_RTOT), smallp(ctx, S_BPREV), ctx->d_flags, rec_dev,
             b, ctx->stream);
  ctx->flags_clean = true;
  if (async) {  // stash A_i, R_tot and the flags for rbl_fetch; no host round trip
    if (!ctx->stash_direct)
      HIPC(hipMemcpyAsync(ctx->h_hist + (size_t)i * rec, ctx->d_stash, rec * sizeof(double),
                          hipMemcpyDeviceToHost, ctx->stream));
    if ((int)ctx->step_ev.size() <= i) ctx->step_ev.resize(i + 1, nullptr);
    if (!ctx->step_ev[i]) HIPC(hipEventCreateWithFlags(&ctx->step_ev[i], hipEventDisableTiming));
    HIPC(hipEventRecord(ctx->step_ev[i], ctx->stream));
    HIPC(hipGetLastError());
    ctx->nblocks = i + 1;
    return RBL_OK;
  }
  if (!ctx->stash_direct)
    HIPC(hipMemcpyAsync(ctx->h_pin, ctx->d_stash, rec * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  int flags[4];
  memcpy(flags, ctx->h_pin + 2 * b * b, sizeof(flags));
  harvest_timers(ctx);
  // row-major device -> column-major host
  for (int r = 0; r < b; ++r)
    for (int c = 0; c < b; ++c) {
      if (A_out) A_out[c * b + r] = ctx->h_pin[r * b + c];
      if (B_out) B_out[c * b + r] = ctx->h_pin[b * b + r * b + c];
    }
  ctx->nblocks = i + 1;
  if (flags[2]) return fail(ctx, RBL_ERR_NUMERIC, "QR breakdown (shifted CholQR failed)");
  return flags[3] ? RBL_WARN_QR_SHIFTED : RBL_OK;
}
// Device -> pageable host copy of a large result (the Ritz vectors, RBL_gpu.jl:219 returns them
// on the host) through two pinned 64 MiB slots: the DMA of piece p runs while host threads copy
// piece p-1 out of the other slot into the caller's memory.  hipMemcpy into pageable memory goes
// through the runtime's own bounce buffer on one thread, well under the PCIe rate (§2: 49-56 GB/s
// pinned).  Every earlier piece's host copy has finished before its slot is refilled.
// RBL_D2H_DIRECT=1 restores the plain copy (A/B).
int d2h_staged(rbl_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (bytes < 4 * kD2HPiece || d2h_direct()) {
    HIPC(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return RBL_OK;
  }
  CHK(ensure_d2h_slots(ctx));
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const char* envt = std::getenv("RBL_D2H_THREADS");
  const int nthr = (int)std::min(envt ? std::max(1u, (unsigned)atoi(envt)) : 8u, hw);
  auto host_copy = [&](size_t p) {
    const size_t off = p * kD2HPiece, len = std::min(kD2HPiece, bytes - off);
    char* d = static_cast<char*>(dst) + off;
    const char* s = static_cast<const char*>(ctx->h_d2h[p & 1]);
    const size_t part = ((len + nthr - 1) / nthr + 4095) & ~size_t(4095);
    std::vector<std::thread> th;
    for (size_t o = part; o < len; o += part)
      th.emplace_back([=] { memcpy(d + o, s + o, std::min(part, len - o)); });
    memcpy(d, s, std::min(part, len));
    for (auto& t : th) t.join();
  };
  const size_t np = (bytes + kD2HPiece - 1) / kD2HPiece;
  for (size_t p = 0; p <= np; ++p) {
    if (p < np) {
      const size_t off = p * kD2HPiece;
      HIPC(hipMemcpyAsync(ctx->h_d2h[p & 1], static_cast<const char*>(src) + off,
                          std::min(kD2HPiece, bytes - off), hipMemcpyDeviceToHost, ctx->stream));
      HIPC(hipEventRecord(ctx->ev_d2h_slot[p & 1], ctx->stream));
    }
    if (p > 0) {
      HIPC(hipEventSynchronize(ctx->ev_d2h_slot[(p - 1) & 1]));
      host_copy(p - 1);
    }
  }
  return RBL_OK;
}

// The Ritz vectors in row pieces with the D2H behind them (rbl_ritz, one chunk of k <= b columns,
// every block resident — fp64, or fp32 where the fp32-input MFMA combination applies — and a
// result of >= 4 staging pieces).  V = [Q_1..Q_m] S and its
// transpose run in kRitzPieces row pieces on a side stream; the staged D2H stays on the context's
// stream, each 64 MiB staging piece issued once the host has seen the row pieces it covers
// finish, so the PCIe copy
// (1.6 GB at ~53 GB/s, 30 ms at C4a) overlaps the basis reads of the later pieces (5.5 ms at 8
// blocks, 17.6 ms at 28) instead of following all of them.  (Copies ordered behind the pieces by
// a device-side stream wait ran at half the PCIe rate in most calls, on either stream:
// profiles/r05_ritz_pipelined_trace_b29.log.)  Piece p (rows [r_p, r_{p+1})) is stored column-major
// with its own row count as leading dimension, so the pieces tile the column-major buffer
// contiguously; the host scatters each staged byte range into V_out's columns.  Every row of V is
// the same sum in the same order as in the one-pass form, so V is bit-identical
// (test_ritz_pipelined_matches_one_pass).  RBL_RITZ_SERIAL=1 restores the one-pass form.
constexpr int kRitzPieces = 8;
int ritz_pipelined(rbl_ctx* ctx, int nblocks, int k, int kcp, const double* d_S, double* pV,
                   double* pVcm, double* V_out) {
  const int b = ctx->b;
  const int64_t nl = ctx->nloc;
  const int64_t pr = (nl / kRitzPieces) & ~int64_t(63);  // rows per piece; the last takes the rest
  int64_t r0p[kRitzPieces + 1];
  for (int p = 0; p < kRitzPieces; ++p) r0p[p] = p * pr;
  r0p[kRitzPieces] = nl;
  CHK(ensure_d2h_slots(ctx));
  CHK(ensure_ritz_stream(ctx));
  HIPC(hipEventRecord(ctx->ev_ritz[kRitzPieces], ctx->stream));  // S is on the device
  HIPC(hipStreamWaitEvent(ctx->rstream, ctx->ev_ritz[kRitzPieces], 0));
  // on every exit, error paths included: the side stream's kernels write U / T and the run
  // scratch, so nothing may leave here with them still queued behind the context's back
  struct DrainSide {
    hipStream_t s;
    ~DrainSide() { (void)hipStreamSynchronize(s); }
  } drain{ctx->rstream};
  {
    StageScope t(ctx, RBL_STAGE_RITZ, ctx->rstream);
    for (int p = 0; p < kRitzPieces; ++p) {
      const int64_t r0 = r0p[p], m = r0p[p + 1] - r0;
      PanelRun X;
      X.stride = ctx->slot;
      X.count = nblocks;
      X.w = b;
      if (ctx->basis_bits == 64) {
        X.base = slotp(ctx, 0) + r0 * b;
        tsmm(m, X, d_S, kcp, pan1(pV + r0 * kcp, kcp), 1.0, 0.0, nullptr, ctx->rstream);
      } else {  // fp32 basis: the fp32-input MFMA form of combine_blocks32, widened on load
        X.base32 = slotp32(ctx, 0) + r0 * b;
        tsmm44_f32x(m, X, d_S, kcp, pan1(pV + r0 * kcp, kcp), 1.0, 0.0, ctx->rstream);
      }
      rowmajor_to_colmajor(pV + r0 * kcp, m, kcp, pVcm + r0 * kcp, ctx->rstream);
      HIPC(hipEventRecord(ctx->ev_ritz[p], ctx->rstream));
    }
  }
  HIPC(hipGetLastError());
  const char* src = reinterpret_cast<const char*>(pVcm);
  const size_t bytes = (size_t)nl * kcp * sizeof(double);
  auto piece_of = [&](size_t o) {  // the row piece holding byte o of the column-major buffer
    int p = 0;
    while (p + 1 < kRitzPieces && (size_t)r0p[p + 1] * kcp * sizeof(double) <= o) ++p;
    return p;
  };
  // device bytes [a, e) of staging piece q (slot q & 1) -> V_out's columns (padding column skipped)
  auto scatter = [&](size_t q, size_t a, size_t e) {
    const char* slot = static_cast<const char*>(ctx->h_d2h[q & 1]);
    const size_t base = q * kD2HPiece;
    for (size_t o = base + a; o < base + e;) {
      const int p = piece_of(o);
      const int64_t r0 = r0p[p], m = r0p[p + 1] - r0;
      const size_t colb = (size_t)m * sizeof(double);
      const size_t within = o - (size_t)r0 * kcp * sizeof(double);
      const size_t c = within / colb, inr = within % colb;
      const size_t run = std::min(base + e, o + (colb - inr));
      if ((int)c < k)
        memcpy(reinterpret_cast<char*>(V_out + (int64_t)c * nl + r0) + inr, slot + (o - base), run - o);
      o = run;
    }
  };
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const char* envt = std::getenv("RBL_D2H_THREADS");
  const int nthr = (int)std::min(envt ? std::max(1u, (unsigned)atoi(envt)) : 8u, hw);
  const size_t nq = (bytes + kD2HPiece - 1) / kD2HPiece;
  int waited = -1;  // the last row piece the context's stream waits for
  for (size_t q = 0; q <= nq; ++q) {
    if (q < nq) {
      const size_t off = q * kD2HPiece, len = std::min(kD2HPiece, bytes - off);
      // the host waits for the pieces, so the copy carries no cross-stream dependency (copies
      // queued behind a hipStreamWaitEvent ran at half the PCIe rate, ~28 GB/s)
      for (const int pl = piece_of(off + len - 1); waited < pl;)
        HIPC(hipEventSynchronize(ctx->ev_ritz[++waited]));
      HIPC(hipMemcpyAsync(ctx->h_d2h[q & 1], src + off, len, hipMemcpyDeviceToHost, ctx->stream));
      HIPC(hipEventRecord(ctx->ev_d2h_slot[q & 1], ctx->stream));
    }
    if (q > 0) {
      const size_t pq = q - 1, len = std::min(kD2HPiece, bytes - pq * kD2HPiece);
      HIPC(hipEventSynchronize(ctx->ev_d2h_slot[pq & 1]));
      const size_t part = ((len + nthr - 1) / nthr + 4095) & ~size_t(4095);
      std::vector<std::thread> th;
      for (size_t o = part; o < len; o += part)
        th.emplace_back([=, &scatter] { scatter(pq, o, std::min(len, o + part)); });
      scatter(pq, 0, std::min(part, len));
      for (auto& t : th) t.join();
    }
  }
  // every piece has finished (the host waited for the last before its copy); later work on the
  // context's stream (the next run's steps reuse U and T) follows the side stream's kernels
  HIPC(hipStreamSynchronize(ctx->rstream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return RBL_OK;
}
}  // namespace

int rbl_ritz(rbl_ctx* ctx, int nblocks, int k, const double* S, double* V_out) {
  if (!ctx || nblocks < 1 || k < 1 || !S) return fail(ctx, RBL_ERR_INVALID, "rbl_ritz: bad arguments");
  if (nblocks > ctx->nblocks) return fail(ctx, RBL_ERR_INVALID, "rbl_ritz: more blocks than computed");
  if (k > nblocks * ctx->b) return fail(ctx, RBL_ERR_INVALID, "rbl_ritz: k > nblocks*b");
  HIPC(hipSetDevice(ctx->device));
  const int b = ctx->b;
  const int64_t rows = (int64_t)nblocks * b;
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  // Ritz columns in chunks of <= 64 (one tsmm44 launch each), halved while a chunk's buffers
  // (S rows, V and its column-major copy) exceed 0.7 of free HBM — RBL_gpu.jl:24-27, 110-125
  // (`blocksize`).  Each chunk reads the basis once.
  size_t free_b = 0, total_b = 0;
  HIPC(hipMemGetInfo(&free_b, &total_b));
  int kc = std::min(k, 64);
  auto chunk_bytes = [&](int w) { return (double)((w + 1) & ~1) * (double)(rows + 2 * nl) * 8.0; };
  while (kc > 1 && chunk_bytes(kc) > 0.7 * (double)free_b) kc = (kc + 1) / 2;
  const int kcp = (kc + 1) & ~1;  // even panel width (16-B row stores), zero-padded column
  if (chunk_bytes(kc) > 0.7 * (double)free_b)
    return fail(ctx, RBL_ERR_OOM, "rbl_ritz: no room for one Ritz column");
  // RBL_RITZ_TRACE=1: host-side split of the call on stderr (diagnostics)
#ifdef RBL_VARIANTS
  const bool trace = std::getenv("RBL_RITZ_TRACE") != nullptr;
#else
  const bool trace = false;
#endif
  auto tnow = [] { return std::chrono::duration<double, std::milli>(
                       std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = trace ? tnow() : 0.0;
  double t_alloc = 0.0, t_comp = 0.0, t_d2h = 0.0;
  // the run's scratch blocks hold a chunk when it is at most b wide (k <= b: every chunk): U
  // (n_local x b) takes V, T the column-major copy, the coefficient buffer (max_blocks b x 2b)
  // the S rows — no 2 x n_local x kcp allocation per call (at C4a 3.2 GB, whose hipMalloc +
  // first touch cost up to ~20 ms of a time-to-k)
  DevBuf<double> own_S, own_V, own_Vcm;
  double *pS = nullptr, *pV = nullptr, *pVcm = nullptr;
  if (kcp <= b && ctx->d_U && ctx->d_T && ctx->d_C && (size_t)rows * kcp <= ctx->C_elems) {
    pS = ctx->d_C;
    pV = ctx->d_U;
    pVcm = ctx->d_T;
  } else {
    HIPC(own_S.alloc(rows * kcp));
    HIPC(own_V.alloc(nl * kcp));
    HIPC(own_Vcm.alloc(nl * kcp));
    pS = own_S;
    pV = own_V;
    pVcm = own_Vcm;
  }
  if (trace) t_alloc = tnow() - t0;
  const bool pipelined = V_out && ctx->nloc > 0 && kc >= k && pV == ctx->d_U &&
                         (ctx->basis_bits == 64 || tsmm44_ok(b, kcp, kcp)) &&
                         nblocks <= ctx->resident && ctx->nloc >= 64 * kRitzPieces &&
                         (size_t)ctx->nloc * kcp * sizeof(double) >= 4 * kD2HPiece &&
                         !d2h_direct() && !ritz_serial();
  std::vector<double> srm((size_t)rows * kcp);
  if (pipelined) {
    for (int64_t r = 0; r < rows; ++r)
      for (int c = 0; c < kcp; ++c) srm[(size_t)r * kcp + c] = c < k ? S[(size_t)c * rows + r] : 0.0;
    HIPC(hipMemcpyAsync(pS, srm.data(), rows * kcp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ctx->path_stats[RBL_PATH_RITZ_PIECES] += 1;
    CHK(ritz_pipelined(ctx, nblocks, k, kcp, pS, pV, pVcm, V_out));
    harvest_timers(ctx);
    if (trace) fprintf(stderr, "rbl_ritz: pipelined, %d row pieces, total %.2f ms\n", kRitzPieces, tnow() - t0);
    return RBL_OK;
  }
  for (int c0 = 0; c0 < k; c0 += kc) {
    const int w = std::min(kc, k - c0);
    // the previous chunk's copy may still read srm (HIP does not promise a pageable source is
    // consumed when hipMemcpyAsync returns): wait for it before refilling
    HIPC(hipStreamSynchronize(ctx->stream));
    // S columns [c0, c0 + w) (column-major, ld = rows) -> row-major rows x kcp, zero-padded
    for (int64_t r = 0; r < rows; ++r)
      for (int c = 0; c < kcp; ++c) srm[(size_t)r * kcp + c] = c < w ? S[(size_t)(c0 + c) * rows + r] : 0.0;
    HIPC(hipMemcpyAsync(pS, srm.data(), rows * kcp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    {
      StageScope t(ctx, RBL_STAGE_RITZ);
      if (ctx->basis_bits == 64) CHK(combine_blocks(ctx, nblocks, kcp, pS, pV));
      else CHK(combine_blocks32(ctx, nblocks, kcp, pS, pV));
    }
    if (ctx->nloc > 0) rowmajor_to_colmajor(pV, ctx->nloc, kcp, pVcm, ctx->stream);
    HIPC(hipGetLastError());
    double tc = 0.0;
    if (trace) {
      HIPC(hipStreamSynchronize(ctx->stream));
      tc = tnow();
      t_comp += tc - t0 - t_alloc - t_comp - t_d2h;
    }
    if (V_out && ctx->nloc > 0)
      CHK(d2h_staged(ctx, V_out + (size_t)c0 * ctx->nloc, pVcm, ctx->nloc * w * sizeof(double)));
    if (trace) {
      HIPC(hipStreamSynchronize(ctx->stream));
      t_d2h += tnow() - tc;
    }
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  if (trace)
    fprintf(stderr, "rbl_ritz: alloc %.2f ms, S + combine + transpose %.2f ms, D2H %.2f ms, total %.2f ms\n",
            t_alloc, t_comp, t_d2h, tnow() - t0);
  return RBL_OK;
}

// ---- Chebyshev-filtered runs ---------------------------------------------------------------
int rbl_set_filter(rbl_ctx* ctx, int degree, double lo, double hi, double ref) {
  if (!ctx) return RBL_ERR_INVALID;
  if (degree < 0) return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter: degree must be >= 0");
  if (degree == 0) {  // clears either kind of filter
    ctx->filt_deg = 0;
    ctx->ser_mu.clear();
    return RBL_OK;
  }
  if (!std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(ref))
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter: lo, hi and ref must be finite");
  if (!(lo < hi)) return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter: needs lo < hi");
  if (ref >= lo && ref <= hi)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter: ref must lie outside the damped interval [lo, hi]");
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter: one rank only (nranks > 1 is not supported)");
  if (ctx->rect)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter: not with a rectangular B (rbl_set_matrix_normal)");
  if (ctx->d_basis32)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter: the fp64 basis only (the current run has basis_bits = 32)");
  ctx->filt_deg = degree;
  ctx->filt_lo = lo;
  ctx->filt_hi = hi;
  ctx->filt_ref = ref;
  ctx->ser_mu.clear();  // replaces a series
  ctx->cloc_step = 0;  // the operator changes: no Gram of an earlier step carries over
  return RBL_OK;
}

int rbl_set_filter_series(rbl_ctx* ctx, int degree, double lo, double hi, const double* mu) {
  if (!ctx) return RBL_ERR_INVALID;
  if (degree < 1 || degree > 65535)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: degree must be in [1, 65535]");
  if (!std::isfinite(lo) || !std::isfinite(hi))
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: lo and hi must be finite");
  if (!(lo < hi)) return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: needs lo < hi");
  if (!mu) return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: mu is NULL");
  for (int j = 0; j <= degree; ++j)
    if (!std::isfinite(mu[j]))
      return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: mu[" + std::to_string(j) + "] is not finite");
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: one rank only (nranks > 1 is not supported)");
  if (ctx->rect)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: not with a rectangular B (rbl_set_matrix_normal)");
  if (ctx->d_basis32)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_filter_series: the fp64 basis only (the current run has basis_bits = 32)");
  ctx->ser_mu.assign(mu, mu + degree + 1);
  ctx->ser_lo = lo;
  ctx->ser_hi = hi;
  ctx->filt_deg = 0;  // replaces a single-polynomial filter
  ctx->cloc_step = 0;  // the operator changes: no Gram of an earlier step carries over
  return RBL_OK;
}

int rbl_apply_filter(rbl_ctx* ctx, int b, const double* X, double* Y) {
  if (!ctx || b < 1 || b > RBL_MAX_BLOCK || !X || !Y)
    return fail(ctx, RBL_ERR_INVALID, "rbl_apply_filter: bad arguments");
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_apply_filter: no matrix");
  if (!has_filter(ctx))
    return fail(ctx, RBL_ERR_STATE, "rbl_apply_filter: no filter set (rbl_set_filter / rbl_set_filter_series)");
  if (ctx->nranks > 1 || ctx->rect)
    return fail(ctx, RBL_ERR_INVALID, "rbl_apply_filter: one rank and a square A only");
  HIPC(hipSetDevice(ctx->device));
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  const size_t padded = (size_t)(nl + kRowPad) * b;
  DevBuf<double> x, xr, y, F[3];
  HIPC(x.alloc(nl * b));
  HIPC(xr.alloc(nl * b));
  for (DevBuf<double>* p : {&y, &F[0], &F[1], &F[2]}) {
    if (p == &F[2] && !has_series(ctx)) continue;  // the series' third block
    HIPC(p->alloc(padded));
    HIPC(hipMemsetAsync(*p, 0, padded * sizeof(double), ctx->stream));
  }
  HIPC(hipMemcpyAsync(x, X, ctx->nloc * b * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  colmajor_to_rowmajor(x, ctx->nloc, b, xr, ctx->stream);
  {
    StageScope t(ctx, RBL_STAGE_AQ);
    CHK(filter_apply(ctx, xr, b, y, F));
  }
  HIPC(hipGetLastError());
  rowmajor_to_colmajor(y, ctx->nloc, b, x, ctx->stream);
  HIPC(hipMemcpyAsync(Y, x, ctx->nloc * b * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  return RBL_OK;
}

// Diagnostics (tools/bench_filter.py --series): hipEvent time per pass of the fused series pass
// (a middle term: reads W, T_{j-1}, T_{j-2}, ACC; writes T_j over W, ACC) and of the pair of
// cheb_axpby launches it replaces (the term, then ACC = ACC + mu T_j), on blocks of `len`
// doubles.  The coefficients keep the values bounded over any number of repeats.
int rbl_bench_series_pass(rbl_ctx* ctx, int64_t len, int reps, double* fused_ms, double* pair_ms) {
  if (!ctx || len < 1 || reps < 1 || !fused_ms || !pair_ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_series_pass: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  DevBuf<double> w, t1, t2, acc;
  const size_t bytes = (size_t)len * sizeof(double);
  for (DevBuf<double>* p : {&w, &t1, &t2, &acc}) {
    HIPC(p->alloc((size_t)len));
    HIPC(hipMemsetAsync(*p, 0, bytes, ctx->stream));
  }
  const double al = 0.5, be = 0.25, mu = 1e-3;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  auto fused = [&] {
    cheb_series_term(len, w, t1, t2, al, be, mu, 0.0, w, acc, false, false, ctx->stream);
  };
  auto pair = [&] {
    cheb_axpby(len, w, t1, t2, al, be, -1.0, w, ctx->stream);
    cheb_axpby(len, acc, w, nullptr, 1.0, mu, 0.0, acc, ctx->stream);  // out may be W
  };
  int st = RBL_OK;
  auto timed = [&](auto&& fn, double* out) {
    fn();  // warm-up
    if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
    for (int r = 0; r < reps; ++r) fn();
    if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
    *out = (double)ms / reps;
  };
  timed(fused, fused_ms);
  timed(pair, pair_ms);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_series_pass: a HIP call failed");
  return RBL_OK;
}

// ---- implicit symmetric low-rank update: the operator A + P S P^T ---------------------------
int rbl_set_lowrank(rbl_ctx* ctx, int r, const double* P, const double* S) {
  if (!ctx) return RBL_ERR_INVALID;
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_lowrank: one rank only (nranks > 1 is not supported)");
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_set_lowrank: no matrix");
  if (ctx->rect)
    return fail(ctx, RBL_ERR_STATE, "rbl_set_lowrank: not with a rectangular B (rbl_set_matrix_normal; "
                                    "its rank-one shift is rbl_set_rect_shift)");
  HIPC(hipSetDevice(ctx->device));
  if (r == 0 || !P) {  // clear: the operator is A again
    HIPC(hipStreamSynchronize(ctx->stream));
    free_lowrank(ctx);
    ctx->cloc_step = 0;
    return RBL_OK;
  }
  if (r < 1 || r > 32) return fail(ctx, RBL_ERR_INVALID, "rbl_set_lowrank: r must be in [1, 32]");
  if (!S) return fail(ctx, RBL_ERR_INVALID, "rbl_set_lowrank: S is NULL");
  if (ctx->d_basis32)
    return fail(ctx, RBL_ERR_STATE, "rbl_set_lowrank: the fp64 basis only (the current run has basis_bits = 32)");
  const int64_t n = ctx->nloc;
  for (int64_t i = 0; i < n * r; ++i)
    if (!std::isfinite(P[i])) return fail(ctx, RBL_ERR_INVALID, "rbl_set_lowrank: P has a non-finite entry");
  for (int i = 0; i < r * r; ++i)
    if (!std::isfinite(S[i])) return fail(ctx, RBL_ERR_INVALID, "rbl_set_lowrank: S has a non-finite entry");
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < i; ++j)
      if (S[i + (size_t)j * r] != S[j + (size_t)i * r])
        return fail(ctx, RBL_ERR_INVALID, "rbl_set_lowrank: S is not symmetric (S[" + std::to_string(i) +
                                              "," + std::to_string(j) + "] != S[" + std::to_string(j) + "," +
                                              std::to_string(i) + "])");
  // P column-major n x r -> row-major n x rp, the padding columns zero
  const int rp = lr_padded_width(r);
  std::vector<double> Pr((size_t)std::max<int64_t>(n, 1) * rp, 0.0);
  for (int j = 0; j < r; ++j)
    for (int64_t i = 0; i < n; ++i) Pr[(size_t)i * rp + j] = P[i + (size_t)j * n];
  HIPC(hipStreamSynchronize(ctx->stream));  // steps in flight still read the old update
  free_lowrank(ctx);
  HIPC(ctx->d_lr_P.alloc(Pr.size()));
  HIPC(ctx->d_lr_S.alloc((size_t)r * r));
  HIPC(hipMemcpy(ctx->d_lr_P, Pr.data(), Pr.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->d_lr_S, S, (size_t)r * r * sizeof(double), hipMemcpyHostToDevice));  // S = S^T
  ctx->lr_r = r;
  ctx->lr_rp = rp;
  ctx->cloc_step = 0;  // the operator changes: no Gram of an earlier step carries over
  return RBL_OK;
}

int rbl_get_lowrank(rbl_ctx* ctx, int* r, double* P_out, double* S_out) {
  if (!ctx) return RBL_ERR_INVALID;
  if (ctx->lr_r == 0) return fail(ctx, RBL_ERR_STATE, "rbl_get_lowrank: no update set");
  HIPC(hipSetDevice(ctx->device));
  if (r) *r = ctx->lr_r;
  const int64_t n = ctx->nloc;
  const int rr = ctx->lr_r, rp = ctx->lr_rp;
  if (P_out) {
    std::vector<double> Pr((size_t)std::max<int64_t>(n, 1) * rp);
    HIPC(hipMemcpy(Pr.data(), ctx->d_lr_P, Pr.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int j = 0; j < rr; ++j)
      for (int64_t i = 0; i < n; ++i) P_out[i + (size_t)j * n] = Pr[(size_t)i * rp + j];
  }
  if (S_out) HIPC(hipMemcpy(S_out, ctx->d_lr_S, (size_t)rr * rr * sizeof(double), hipMemcpyDeviceToHost));
  return RBL_OK;
}

// Diagnostics: hipEvent time per pass of the projection w = P^T X (with its reduce_slab) and of
// the update U += P c, on scratch blocks of rows x b (X, U) and rows x lr_padded_width(r) (P)
// allocated and zeroed for the call.
int rbl_bench_lowrank_pass(rbl_ctx* ctx, int64_t rows, int b, int r, int reps, double* project_ms,
                           double* update_ms) {
  if (!ctx || rows < 1 || b < 1 || b > RBL_MAX_BLOCK || r < 1 || r > 32 || reps < 1 || !project_ms ||
      !update_ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_lowrank_pass: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  const int rp = lr_padded_width(r);
  const size_t grid = (size_t)lr_project_grid(rows, b, rp);
  DevBuf<double> x, u, p, wc, part;
  const std::pair<DevBuf<double>*, size_t> bufs[] = {{&x, (size_t)rows * b},
                                             {&u, (size_t)rows * b},
                                             {&p, (size_t)rows * rp},
                                             {&wc, (size_t)2 * rp * b},
                                             {&part, grid * rp * b}};
  for (const auto& q : bufs) {
    HIPC(q.first->alloc(q.second));
    HIPC(hipMemsetAsync(*q.first, 0, q.second * sizeof(double), ctx->stream));
  }
  double *w = wc, *c = wc + (size_t)rp * b;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  auto project = [&] { lr_project(rows, b, rp, p, x, part, w, ctx->stream); };
  auto update = [&] { lr_update(rows, b, rp, p, c, u, ctx->stream); };
  int st = RBL_OK;
  auto timed = [&](auto&& fn, double* out) {
    fn();  // warm-up
    if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
    for (int q = 0; q < reps; ++q) fn();
    if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
    *out = (double)ms / reps;
  };
  timed(project, project_ms);
  timed(update, update_ms);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_lowrank_pass: a HIP call failed");
  return RBL_OK;
}

// ---- preconditioned conjugate gradients: (Op + shift I) X = B -----------------------------------
int rbl_set_precond_lowrank(rbl_ctx* ctx, int r, const double* V, const double* dv) {
  if (!ctx) return RBL_ERR_INVALID;
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_precond_lowrank: one rank only (nranks > 1 is not supported)");
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_set_precond_lowrank: no matrix");
  if (ctx->rect)
    return fail(ctx, RBL_ERR_INVALID, "rbl_set_precond_lowrank: not with a rectangular B (rbl_set_matrix_normal)");
  if (r < 1 || r > 32) return fail(ctx, RBL_ERR_INVALID, "rbl_set_precond_lowrank: r must be in [1, 32]");
  if (!V || !dv) return fail(ctx, RBL_ERR_INVALID, "rbl_set_precond_lowrank: V or dv is NULL");
  const int64_t n = ctx->nloc;
  for (int64_t i = 0; i < n * r; ++i)
    if (!std::isfinite(V[i])) return fail(ctx, RBL_ERR_INVALID, "rbl_set_precond_lowrank: V has a non-finite entry");
  for (int i = 0; i < r; ++i)
    if (!std::isfinite(dv[i]) || !(dv[i] > -1.0))
      return fail(ctx, RBL_ERR_INVALID, "rbl_set_precond_lowrank: dv[" + std::to_string(i) +
                                            "] must be finite and > -1 (I + V diag(dv) V^T positive definite)");
  HIPC(hipSetDevice(ctx->device));
  // V column-major n x r -> row-major n x rp, the padding columns zero
  const int rp = lr_padded_width(r);
  std::vector<double> Vr((size_t)std::max<int64_t>(n, 1) * rp, 0.0), dvp((size_t)rp, 0.0);
  for (int j = 0; j < r; ++j)
    for (int64_t i = 0; i < n; ++i) Vr[(size_t)i * rp + j] = V[i + (size_t)j * n];
  std::copy(dv, dv + r, dvp.begin());
  HIPC(hipStreamSynchronize(ctx->stream));
  PrecondBufs nb;  // the context keeps its preconditioner unless every step below succeeds
  HIPC(nb.d_pc_V.alloc(Vr.size()));
  HIPC(nb.d_pc_dv.alloc(dvp.size()));
  HIPC(hipMemcpy(nb.d_pc_V, Vr.data(), Vr.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(nb.d_pc_dv, dvp.data(), dvp.size() * sizeof(double), hipMemcpyHostToDevice));
  static_cast<PrecondBufs&>(*ctx) = std::move(nb);
  ctx->pc_r = r;
  ctx->pc_rp = rp;
  return RBL_OK;
}

int rbl_clear_precond(rbl_ctx* ctx) {
  if (!ctx) return RBL_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  free_precond(ctx);
  return RBL_OK;
}

namespace {

// Every device buffer of one rbl_solve / rbl_bench_cg_pass call: released on every return path.
struct CgBufs {
  DevBuf<double> B, X, R, P, W;  // n x b row-major blocks, (n_local + kRowPad) x b, zeroed
  DevBuf<double> part;           // workgroup partials of a pass (cg_grid x 2 b)
  DevBuf<double> dots;           // their sums (2 b)
  DevBuf<double> sc;             // rho, alpha, beta, |b|^2, |r|^2 (b each)
  DevBuf<int> isc;               // iters (b), status (b), nactive (1)
  DevBuf<double> hist;           // (alpha, beta) per iteration (2 max_iter b), or empty
  DevBuf<double> wc;             // preconditioner: w = V^T r and c = dv o w (rp x b each)
  DevBuf<double> lrpart;         //   and the workgroup partials of w
  CgScalars scalars(int b) const {
    CgScalars s;
    s.rho = sc;
    s.alpha = sc + b;
    s.beta = sc + 2 * b;
    s.bb = sc + 3 * b;
    s.rr = sc + 4 * b;
    s.iters = isc;
    s.status = isc + b;
    s.nactive = isc + 2 * b;
    s.hist = hist;
    return s;
  }
};

int cg_alloc(rbl_ctx* ctx, CgBufs& g, int64_t rows, int b, int rp, size_t hist_len) {
  const size_t padded = (size_t)(std::max<int64_t>(rows, 1) + kRowPad) * b;
  for (DevBuf<double>* p : {&g.B, &g.X, &g.R, &g.P, &g.W}) {
    HIPC(p->alloc(padded));
    HIPC(hipMemsetAsync(*p, 0, padded * sizeof(double), ctx->stream));
  }
  HIPC(g.part.alloc((size_t)cg_grid(rows, b) * 2 * b));
  HIPC(g.dots.alloc((size_t)2 * b));
  HIPC(g.sc.alloc((size_t)5 * b));
  HIPC(hipMemsetAsync(g.sc, 0, (size_t)5 * b * sizeof(double), ctx->stream));
  HIPC(g.isc.alloc((size_t)2 * b + 1));
  HIPC(hipMemsetAsync(g.isc, 0, ((size_t)2 * b + 1) * sizeof(int), ctx->stream));
  if (hist_len) {
    HIPC(g.hist.alloc(hist_len));
    HIPC(hipMemsetAsync(g.hist, 0, hist_len * sizeof(double), ctx->stream));
  }
  if (rp > 0) {
    HIPC(g.wc.alloc((size_t)2 * rp * b));
    HIPC(hipMemsetAsync(g.wc, 0, (size_t)2 * rp * b * sizeof(double), ctx->stream));
    HIPC(g.lrpart.alloc((size_t)lr_project_grid(rows, b, rp) * rp * b));
  }
  return RBL_OK;
}

}  // namespace

int rbl_solve(rbl_ctx* ctx, int b, const double* B, double* X, double shift, double tol, int max_iter,
              int check_every, int use_x0, int* iters, int* status, double* resid, double* coef) {
  if (!ctx) return RBL_ERR_INVALID;
  if (b < 1 || b > RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "rbl_solve: b must be in [1," + std::to_string(RBL_MAX_BLOCK) + "]");
  if (!B || !X || !iters || !status || !resid)
    return fail(ctx, RBL_ERR_INVALID, "rbl_solve: B, X, iters, status or resid is NULL");
  if (!std::isfinite(shift)) return fail(ctx, RBL_ERR_INVALID, "rbl_solve: shift must be finite");
  if (!std::isfinite(tol) || !(tol > 0.0) || !(tol < 1.0))
    return fail(ctx, RBL_ERR_INVALID, "rbl_solve: tol must be in (0, 1)");
  if (max_iter < 1 || max_iter > 65535)
    return fail(ctx, RBL_ERR_INVALID, "rbl_solve: max_iter must be in [1, 65535]");
  if (coef && max_iter > 4096)
    return fail(ctx, RBL_ERR_INVALID, "rbl_solve: with a coefficient history max_iter must be <= 4096");
  if (check_every < 1) return fail(ctx, RBL_ERR_INVALID, "rbl_solve: check_every must be >= 1");
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_solve: one rank only (nranks > 1 is not supported)");
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_solve: no matrix");
  if (ctx->rect)
    return fail(ctx, RBL_ERR_INVALID, "rbl_solve: not with a rectangular B (rbl_set_matrix_normal)");
  if (ctx->d_basis32)
    return fail(ctx, RBL_ERR_STATE, "rbl_solve: the fp64 basis only (the current run has basis_bits = 32)");
  HIPC(hipSetDevice(ctx->device));
  const int64_t n = ctx->nloc;
  const int rp = ctx->pc_rp;
  const size_t hist_len = coef ? (size_t)2 * max_iter * b : 0;
  CgBufs g;
  CHK(cg_alloc(ctx, g, n, b, rp, hist_len));
  const CgScalars sc = g.scalars(b);
  double *w = g.wc, *c = rp > 0 ? g.wc + (size_t)rp * b : nullptr;
  hipStream_t st = ctx->stream;
  // column-major host blocks pass through W, which the first product overwrites
  HIPC(hipMemcpyAsync(g.W, B, n * b * sizeof(double), hipMemcpyHostToDevice, st));
  colmajor_to_rowmajor(g.W, n, b, g.B, st);
  if (use_x0) {
    HIPC(hipMemcpyAsync(g.W, X, n * b * sizeof(double), hipMemcpyHostToDevice, st));
    colmajor_to_rowmajor(g.W, n, b, g.X, st);
  }
  HIPC(hipGetLastError());
  auto product = [&](const double* in) -> int {
    StageScope t(ctx, RBL_STAGE_AQ);
    const int s = apply_A(ctx, in, 0, b, g.W, nullptr, nullptr, nullptr);
    return s < 0 ? s : RBL_OK;
  };
  // z = M^-1 r through the small quantities: w = V^T r, c = dv o w
  auto precond = [&] {
    if (rp == 0) return;
    lr_project(n, b, rp, ctx->d_pc_V, g.R, g.lrpart, w, st);
    cg_small(rp, b, ctx->d_pc_dv, w, c, st);
  };
  int nactive = 0;
  auto read_active = [&]() -> int {
    HIPC(hipMemcpyAsync(&nactive, sc.nactive, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    harvest_timers(ctx);
    return RBL_OK;
  };
  const double tol2 = tol * tol;
  // with stage timers on, every iteration takes four events from the context's pool, and only a
  // harvest after a synchronisation returns them: the host then looks at the active count at least
  // every kCgTimedCheck iterations whatever check_every is (the result does not depend on it)
  constexpr int kCgTimedCheck = 64;
  const int every = ctx->timers ? std::min(check_every, kCgTimedCheck) : check_every;
  if (use_x0) CHK(product(g.X));
  {
    StageScope t(ctx, RBL_STAGE_3TERM);
    cg_resid(n, b, g.B, g.W, use_x0 ? g.X.p : nullptr, shift, g.R, g.part, g.dots, st);
    precond();
    cg_beta(b, rp, true, 0, g.dots, w, c, tol2, sc, st);
    cg_dir(n, b, rp, g.R, g.P, ctx->d_pc_V, c, sc, st);  // beta = 0, P zeroed: p = z
  }
  HIPC(hipGetLastError());
  CHK(read_active());
  for (int j = 0; j < max_iter && nactive > 0; ++j) {
    CHK(product(g.P));
    {
      StageScope t(ctx, RBL_STAGE_3TERM);
      cg_dot(n, b, g.P, g.W, shift, g.part, g.dots, st);
      cg_alpha(b, g.dots, sc, st);
      cg_update(n, b, g.X, g.R, g.P, g.W, shift, sc, g.part, g.dots, st);
      precond();
      cg_beta(b, rp, false, j, g.dots, w, c, tol2, sc, st);
      cg_dir(n, b, rp, g.R, g.P, ctx->d_pc_V, c, sc, st);
    }
    HIPC(hipGetLastError());
    if ((j + 1) % every == 0 && j + 1 < max_iter) CHK(read_active());
  }
  // the true residual b - (Op + shift I) x from the device-resident B (into P, no longer needed)
  CHK(product(g.X));
  {
    StageScope t(ctx, RBL_STAGE_3TERM);
    cg_resid(n, b, g.B, g.W, g.X, shift, g.P, g.part, g.dots, st);
  }
  HIPC(hipGetLastError());
  std::vector<double> dots((size_t)2 * b), hist(hist_len);
  std::vector<int> isc((size_t)2 * b + 1);
  rowmajor_to_colmajor(g.X, n, b, g.W, st);
  HIPC(hipMemcpyAsync(X, g.W, n * b * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(dots.data(), g.dots, dots.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(isc.data(), g.isc, isc.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  if (hist_len) HIPC(hipMemcpyAsync(hist.data(), g.hist, hist_len * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  harvest_timers(ctx);
  for (int col = 0; col < b; ++col) {
    iters[col] = isc[col];
    const int s = isc[(size_t)b + col];
    status[col] = s == kCgActive ? RBL_SOLVE_MAX_ITER : s;
    const double bb = dots[col], rr = dots[(size_t)b + col];
    resid[col] = bb > 0.0 ? std::sqrt(rr / bb) : std::sqrt(rr);
    if (coef)
      for (int j = 0; j < max_iter; ++j)
        for (int q = 0; q < 2; ++q)
          coef[(size_t)col * 2 * max_iter + 2 * j + q] = hist[((size_t)2 * j + q) * b + col];
  }
  return RBL_OK;
}

// Diagnostics (tools/bench_solve.py): hipEvent time per pass of the three row passes of one CG
// iteration on scratch blocks of len_rows x b doubles — ms[0] the dot pass, ms[1] the update pass
// (each with its reduce_slab), ms[2] the direction pass; with r > 0 the direction pass reads a V of
// lr_padded_width(r) columns and ms[2] includes the projection w = V^T r and c = dv o w before it.
// All columns stay active; alpha = beta = 0 keeps the values bounded over any number of repeats.
int rbl_bench_cg_pass(rbl_ctx* ctx, int64_t len_rows, int b, int r, int reps, double* ms) {
  if (!ctx || len_rows < 1 || b < 1 || b > RBL_MAX_BLOCK || r < 0 || r > 32 || reps < 1 || !ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_cg_pass: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  const int rp = r > 0 ? lr_padded_width(r) : 0;
  CgBufs g;
  CHK(cg_alloc(ctx, g, len_rows, b, rp, 0));
  DevBuf<double> V, dv;
  if (rp > 0) {
    HIPC(V.alloc((size_t)len_rows * rp));
    HIPC(hipMemsetAsync(V, 0, (size_t)len_rows * rp * sizeof(double), ctx->stream));
    HIPC(dv.alloc((size_t)rp));
    HIPC(hipMemsetAsync(dv, 0, (size_t)rp * sizeof(double), ctx->stream));
  }
  const CgScalars sc = g.scalars(b);
  std::vector<int> act((size_t)b, kCgActive);
  HIPC(hipMemcpyAsync(sc.status, act.data(), (size_t)b * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  double *w = g.wc, *c = rp > 0 ? g.wc + (size_t)rp * b : nullptr;
  hipStream_t st = ctx->stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  auto dot = [&] { cg_dot(len_rows, b, g.P, g.W, 0.5, g.part, g.dots, st); };
  auto update = [&] { cg_update(len_rows, b, g.X, g.R, g.P, g.W, 0.5, sc, g.part, g.dots, st); };
  auto dir = [&] {
    if (rp > 0) {
      lr_project(len_rows, b, rp, V, g.R, g.lrpart, w, st);
      cg_small(rp, b, dv, w, c, st);
    }
    cg_dir(len_rows, b, rp, g.R, g.P, V, c, sc, st);
  };
  int stt = RBL_OK;
  auto timed = [&](auto&& fn, double* out) {
    fn();  // warm-up
    if (hipEventRecord(e0, st) != hipSuccess) stt = RBL_ERR_HIP;
    for (int q = 0; q < reps; ++q) fn();
    if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) stt = RBL_ERR_HIP;
    float el = 0.f;
    if (hipEventElapsedTime(&el, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) stt = RBL_ERR_HIP;
    *out = (double)el / reps;
  };
  timed(dot, &ms[0]);
  timed(update, &ms[1]);
  timed(dir, &ms[2]);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (stt != RBL_OK) return fail(ctx, stt, "rbl_bench_cg_pass: a HIP call failed");
  return RBL_OK;
}

// ---- Chebyshev moments (kernel polynomial method) ------------------------------------------
// m_j = x_c^T T_j((A - cI)/e) x_c, j = 0..2 degree, from degree SpMMs: t_j = T_j x by the
// recurrence and scalars of series_apply, and the product identities
//     m_0 = <x,x>,  m_1 = <t_1,x>,  m_{2j} = 2 <t_j,t_j> - m_0,  m_{2j-1} = 2 <t_j,t_{j-1}> - m_1.
// The blocks are the call's own: t_j lives in buf[j % 3] with x = t_0 in buf[0]; term j's SpMM
// writes W = A t_{j-1} over t_{j-3} (dead by then) and cheb_moment_term turns W into t_j in place
// while it forms the partials of the two dots, which reduce_slab adds into the term's slot of
// `dots` (term 1: [tt, tp, xx], 3b; term j >= 2: [tt, tp], 2b).  One D2H at the end; the doubling
// finishes here in float64.
int rbl_cheb_moments(rbl_ctx* ctx, int b, int degree, double lo, double hi, const double* X,
                     uint64_t seed, double* mom_out) {
  if (!ctx) return RBL_ERR_INVALID;
  if (b < 1 || b > RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_moments: b must be in [1," + std::to_string(RBL_MAX_BLOCK) + "]");
  if (degree < 1 || degree > 65535)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_moments: degree must be in [1, 65535]");
  if (!std::isfinite(lo) || !std::isfinite(hi))
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_moments: lo and hi must be finite");
  if (!(lo < hi)) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_moments: needs lo < hi");
  if (!mom_out) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_moments: mom_out is NULL");
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_moments: one rank only (nranks > 1 is not supported)");
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_cheb_moments: no matrix");
  if (ctx->rect)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_moments: not with a rectangular B (rbl_set_matrix_normal)");
  HIPC(hipSetDevice(ctx->device));
  const int64_t n = ctx->nloc, nl = std::max<int64_t>(n, 1);
  const size_t padded = (size_t)(nl + kRowPad) * b;
  const size_t nmom = (size_t)(2 * degree + 1) * b;
  const int grid = moment_grid(n, b);
  DevBuf<double> f[3], slab, dots;
  for (DevBuf<double>& p : f) {
    HIPC(p.alloc(padded));
    HIPC(hipMemsetAsync(p, 0, padded * sizeof(double), ctx->stream));
  }
  HIPC(slab.alloc((size_t)grid * 3 * b));
  HIPC(dots.alloc(nmom));
  if (X) {  // column-major through f[1], which the first SpMM overwrites
    HIPC(hipMemcpyAsync(f[1], X, n * b * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    colmajor_to_rowmajor(f[1], n, b, f[0], ctx->stream);
  } else {
    randn_block(f[0], n, b, ctx->r0, seed, ctx->stream, ctx->relabeled ? &ctx->relabel_perm : nullptr);
  }
  HIPC(hipGetLastError());
  const double c = 0.5 * (lo + hi), e = 0.5 * (hi - lo);
  {
    StageScope t(ctx, RBL_STAGE_AQ);
    const double* t1 = f[0];  // t_{j-1}
    const double* t2 = nullptr;   // t_{j-2}
    double* dj = dots;
    for (int j = 1; j <= degree; ++j) {
      double* tj = f[j % 3];
      const int st = apply_A(ctx, t1, 0, b, tj, nullptr, nullptr, nullptr);
      if (st < 0) return st;
      const double al = (j == 1 ? 1.0 : 2.0) / e;
      const int nq = j == 1 ? 3 : 2;
      cheb_moment_term(n, b, tj, t1, t2, al, -al * c, tj, slab, grid, j == 1, j == degree, ctx->stream);
      reduce_slab(slab, grid, (int64_t)nq * b, dj, nullptr, ctx->stream);
      HIPC(hipGetLastError());
      dj += (size_t)nq * b;
      t2 = t1;
      t1 = tj;
    }
  }
  std::vector<double> d(nmom);
  HIPC(hipMemcpyAsync(d.data(), dots, nmom * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  const size_t ld = (size_t)2 * degree + 1;
  for (int col = 0; col < b; ++col) {
    double* m = mom_out + ld * col;
    const double m0 = d[(size_t)2 * b + col], m1 = d[(size_t)b + col];
    m[0] = m0;
    m[1] = m1;
    m[2] = 2.0 * d[col] - m0;
    for (int j = 2; j <= degree; ++j) {
      const double* dj = d.data() + (size_t)3 * b + (size_t)(j - 2) * 2 * b;
      m[2 * j] = 2.0 * dj[col] - m0;
      m[2 * j - 1] = 2.0 * dj[b + col] - m1;
    }
  }
  return RBL_OK;
}

// Diagnostics (tools/bench_filter.py --moments): hipEvent time per pass of the moment pass (a
// middle term: reads W, t_{j-1}, t_{j-2}; writes t_j over W and the workgroup partials), its
// reduce_slab included, on blocks of len_rows x b doubles.  The coefficients keep the values
// bounded over any number of repeats.
int rbl_bench_moment_pass(rbl_ctx* ctx, int64_t len_rows, int b, int reps, double* ms) {
  if (!ctx || len_rows < 1 || b < 1 || b > RBL_MAX_BLOCK || reps < 1 || !ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_moment_pass: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  const int grid = moment_grid(len_rows, b);
  DevBuf<double> w, t1, t2, slab, dots;
  const size_t bytes = (size_t)len_rows * b * sizeof(double);
  for (DevBuf<double>* p : {&w, &t1, &t2}) {
    HIPC(p->alloc((size_t)len_rows * b));
    HIPC(hipMemsetAsync(*p, 0, bytes, ctx->stream));
  }
  HIPC(slab.alloc((size_t)grid * 2 * b));
  HIPC(dots.alloc((size_t)2 * b));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  auto pass = [&] {
    cheb_moment_term(len_rows, b, w, t1, t2, 0.5, 0.25, w, slab, grid, false, false,
                     ctx->stream);
    reduce_slab(slab, grid, (int64_t)2 * b, dots, nullptr, ctx->stream);
  };
  int st = RBL_OK;
  pass();  // warm-up
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int r = 0; r < reps; ++r) pass();
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float el = 0.f;
  if (hipEventElapsedTime(&el, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)el / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_moment_pass: a HIP call failed");
  return RBL_OK;
}

// ---- diagonals of Chebyshev series (matrix functions) ----------------------------------------
// num[row][e] = sum_c x_c[row] (p_e(Op) x_c)[row], p_e = sum_j coef[j][e] T_j((Op - cI)/e), and
// den[row] = sum_c x_c[row]^2, from `degree` SpMMs for all nf series: the recurrence and scalars of
// rbl_cheb_moments, each term followed by ONE cheb_diag_term that forms t_j, the row sums of X o t_j
// and the nf updates of D.  The blocks are the call's own: X stays in xb (the rotation of the three
// work blocks overwrites t_0's slot at term 3, and every term reads X); t_j lives in f[j % 3].
int rbl_cheb_diag(rbl_ctx* ctx, int b, int degree, double lo, double hi, int nf, const double* coef,
                  const double* X, uint64_t seed, int probe, double* num_out, double* den_out) {
  if (!ctx) return RBL_ERR_INVALID;
  if (b < 1 || b > 256) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: b must be in [1, 256]");
  if (degree < 1 || degree > 65535)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: degree must be in [1, 65535]");
  if (nf < 1 || nf > 32) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: nf must be in [1, 32]");
  if (!std::isfinite(lo) || !std::isfinite(hi))
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: lo and hi must be finite");
  if (!(lo < hi)) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: needs lo < hi");
  if (!coef) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: coef is NULL");
  if (probe != RBL_PROBE_GAUSS && probe != RBL_PROBE_SIGN)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: probe must be RBL_PROBE_GAUSS or RBL_PROBE_SIGN");
  if (!num_out || !den_out) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: num_out or den_out is NULL");
  const size_t ncoef = (size_t)(degree + 1) * nf;
  for (size_t i = 0; i < ncoef; ++i)
    if (!std::isfinite(coef[i])) return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: coef has a non-finite entry");
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: one rank only (nranks > 1 is not supported)");
  if (!has_matrix(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_cheb_diag: no matrix");
  if (ctx->rect)
    return fail(ctx, RBL_ERR_INVALID, "rbl_cheb_diag: not with a rectangular B (rbl_set_matrix_normal)");
  HIPC(hipSetDevice(ctx->device));
  const int64_t n = ctx->nloc, nl = std::max<int64_t>(n, 1);
  const size_t padded = (size_t)(nl + kRowPad) * b;
  // term-major on the device: term j's nf coefficients contiguous
  std::vector<double> cj(ncoef);
  for (int e = 0; e < nf; ++e)
    for (int j = 0; j <= degree; ++j) cj[(size_t)j * nf + e] = coef[(size_t)e * (degree + 1) + j];
  DevBuf<double> f[3], xb, dd, dcm, dq, dcoef;
  for (DevBuf<double>* p : {&f[0], &f[1], &f[2], &xb}) {
    HIPC(p->alloc(padded));
    HIPC(hipMemsetAsync(*p, 0, padded * sizeof(double), ctx->stream));
  }
  HIPC(dd.alloc((size_t)nl * nf));
  HIPC(dcm.alloc((size_t)nl * nf));
  HIPC(dq.alloc((size_t)nl));
  HIPC(dcoef.alloc(ncoef));
  HIPC(hipMemcpyAsync(dcoef, cj.data(), ncoef * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (X) {  // column-major through f[1], which the first SpMM overwrites
    HIPC(hipMemcpyAsync(f[1], X, n * b * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    colmajor_to_rowmajor(f[1], n, b, xb, ctx->stream);
  } else {
    randn_block(xb, n, b, ctx->r0, seed, ctx->stream, ctx->relabeled ? &ctx->relabel_perm : nullptr);
    if (probe == RBL_PROBE_SIGN) sign_block(n * b, xb, ctx->stream);
  }
  HIPC(hipGetLastError());
  const double c = 0.5 * (lo + hi), e = 0.5 * (hi - lo);
  {
    StageScope t(ctx, RBL_STAGE_AQ);
    const double* t1 = xb;   // t_{j-1}
    const double* t2 = nullptr;  // t_{j-2}
    for (int j = 1; j <= degree; ++j) {
      double* tj = f[j % 3];
      const int st = apply_A(ctx, t1, 0, b, tj, nullptr, nullptr, nullptr);
      if (st < 0) return st;
      const double al = (j == 1 ? 1.0 : 2.0) / e;
      const double* cf = dcoef + (j == 1 ? 0 : (size_t)j * nf);
      cheb_diag_term(n, b, nf, tj, t1, t2, xb, al, -al * c, tj, cf, dd, dq, j == 1, j == degree,
                     ctx->stream);
      HIPC(hipGetLastError());
      t2 = t1;
      t1 = tj;
    }
  }
  rowmajor_to_colmajor(dd, n, nf, dcm, ctx->stream);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(num_out, dcm, n * nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipMemcpyAsync(den_out, dq, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  return RBL_OK;
}

// Diagnostics (tools/bench_funm.py): hipEvent time per pass of the diagonal pass (a middle term:
// reads W, t_{j-1}, t_{j-2}, X; writes t_j over W; read-modify-write of D) on blocks of
// len_rows x b doubles and a len_rows x nf D.  The coefficients keep the values bounded over any
// number of repeats.
int rbl_bench_diag_pass(rbl_ctx* ctx, int64_t len_rows, int b, int nf, int reps, double* ms) {
  if (!ctx || len_rows < 1 || b < 1 || b > 256 || nf < 1 || nf > 32 || reps < 1 || !ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_diag_pass: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  DevBuf<double> w, t1, t2, x, dd, dq, dcoef;
  const size_t bytes = (size_t)len_rows * b * sizeof(double);
  for (DevBuf<double>* p : {&w, &t1, &t2, &x}) {
    HIPC(p->alloc((size_t)len_rows * b));
    HIPC(hipMemsetAsync(*p, 0, bytes, ctx->stream));
  }
  HIPC(dd.alloc((size_t)len_rows * nf));
  HIPC(hipMemsetAsync(dd, 0, (size_t)len_rows * nf * sizeof(double), ctx->stream));
  HIPC(dq.alloc((size_t)len_rows));
  HIPC(dcoef.alloc((size_t)nf));
  const std::vector<double> cf((size_t)nf, 1e-3);
  HIPC(hipMemcpyAsync(dcoef, cf.data(), (size_t)nf * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  auto pass = [&] {
    cheb_diag_term(len_rows, b, nf, w, t1, t2, x, 0.5, 0.25, w, dcoef, dd, dq,
                   false, false, ctx->stream);
  };
  int st = RBL_OK;
  pass();  // warm-up
  if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
  for (int r = 0; r < reps; ++r) pass();
  if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
  float el = 0.f;
  if (hipEventElapsedTime(&el, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
  *ms = (double)el / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_diag_pass: a HIP call failed");
  return RBL_OK;
}

// ---- Rayleigh-Ritz on A -------------------------------------------------------------------
int rbl_ritz_project(rbl_ctx* ctx, int nblocks, int k, const double* S, double* H_out) {
  if (!ctx || nblocks < 1 || k < 1 || !S || !H_out)
    return fail(ctx, RBL_ERR_INVALID, "rbl_ritz_project: bad arguments");
  if (k > RBL_MAX_BLOCK)
    return fail(ctx, RBL_ERR_INVALID, "rbl_ritz_project: k must be <= " + std::to_string(RBL_MAX_BLOCK));
  if (ctx->nranks > 1) return fail(ctx, RBL_ERR_INVALID, "rbl_ritz_project: one rank only");
  if (!ctx->d_basis && !ctx->d_basis32) return fail(ctx, RBL_ERR_STATE, "rbl_ritz_project before rbl_start");
  if (nblocks > ctx->nblocks) return fail(ctx, RBL_ERR_INVALID, "rbl_ritz_project: more blocks than computed");
  if (k > nblocks * ctx->b) return fail(ctx, RBL_ERR_INVALID, "rbl_ritz_project: k > nblocks*b");
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->d_rv.reset();
  ctx->d_rw.reset();
  ctx->ritz_k = 0;
  const int b = ctx->b;
  const int kp = (k + 1) & ~1;  // even width (16-B row stores), the pad column zero
  const int64_t rows = (int64_t)nblocks * b;
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  const size_t vbytes = (size_t)(nl + kRowPad) * kp * sizeof(double);
  HIPC(ctx->d_rv.alloc((size_t)(nl + kRowPad) * kp));
  HIPC(ctx->d_rw.alloc((size_t)(nl + kRowPad) * kp));
  HIPC(hipMemsetAsync(ctx->d_rv, 0, vbytes, ctx->stream));
  HIPC(hipMemsetAsync(ctx->d_rw, 0, vbytes, ctx->stream));
  // V = [Q_1..Q_nblocks] S, kept on the device
  std::vector<double> srm((size_t)rows * kp);
  for (int64_t r = 0; r < rows; ++r)
    for (int c = 0; c < kp; ++c) srm[(size_t)r * kp + c] = c < k ? S[(size_t)c * rows + r] : 0.0;
  DevBuf<double> dS;
  HIPC(dS.alloc(rows * kp));
  HIPC(hipMemcpyAsync(dS, srm.data(), rows * kp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  {
    StageScope t(ctx, RBL_STAGE_RITZ);
    if (ctx->basis_bits == 64) CHK(combine_blocks(ctx, nblocks, kp, dS, ctx->d_rv));
    else CHK(combine_blocks32(ctx, nblocks, kp, dS, ctx->d_rv));
  }
  // W = A V with the plain operator, in column chunks of the run's block size where that is
  // one the MFMA SpMM kernels take (b in {16, 32}; the only widths left once the CSR is
  // released), else all columns at once through the kernel rbl_spmm_kernel_for(kp) names
  {
    StageScope t(ctx, RBL_STAGE_AQ);
    const int cw = (b == 16 || b == 32) ? b : kp;
    if (cw == kp) {
      const int st = apply_A(ctx, ctx->d_rv, 0, kp, ctx->d_rw, nullptr, nullptr, nullptr);
      if (st < 0) return st;
    } else {
      const size_t cbytes = (size_t)(nl + kRowPad) * cw * sizeof(double);
      DevBuf<double> xc, yc;
      HIPC(xc.alloc((size_t)(nl + kRowPad) * cw));
      HIPC(yc.alloc((size_t)(nl + kRowPad) * cw));
      HIPC(hipMemsetAsync(xc, 0, cbytes, ctx->stream));
      HIPC(hipMemsetAsync(yc, 0, cbytes, ctx->stream));
      for (int c0 = 0; c0 < kp; c0 += cw) {
        const int w = std::min(cw, kp - c0);
        if (w < cw && c0 > 0) HIPC(hipMemsetAsync(xc, 0, cbytes, ctx->stream));
        copy_cols(ctx->nloc, w, ctx->d_rv, kp, c0, xc, cw, 0, ctx->stream);
        const int st = apply_A(ctx, xc, 0, cw, yc, nullptr, nullptr, nullptr);
        if (st < 0) return st;
        copy_cols(ctx->nloc, w, yc, cw, 0, ctx->d_rw, kp, c0, ctx->stream);
      }
      HIPC(hipGetLastError());
      HIPC(hipStreamSynchronize(ctx->stream));  // the chunk blocks leave scope
    }
    HIPC(hipGetLastError());
  }
  // H = V^T W
  std::vector<double> h((size_t)kp * kp, 0.0);
  if (ctx->nloc > 0) {
    StageScope t(ctx, RBL_STAGE_RITZ);
    const int splits = gram_splits(ctx->nloc, 1, kp, kp);
    DevBuf<double> slab, dH;
    HIPC(slab.alloc((size_t)splits * kp * kp));
    HIPC(dH.alloc((size_t)kp * kp));
    gram_partial(ctx->nloc, run1(ctx->d_rv, kp), pan1(ctx->d_rw, kp), slab, splits, nullptr, ctx->stream);
    reduce_slab(slab, splits, (int64_t)kp * kp, dH, nullptr, ctx->stream);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(h.data(), dH, (size_t)kp * kp * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  for (int r = 0; r < k; ++r)
    for (int c = 0; c < k; ++c) H_out[(size_t)c * k + r] = h[(size_t)r * kp + c];
  ctx->ritz_k = k;
  return RBL_OK;
}

int rbl_ritz_finish(rbl_ctx* ctx, int k, const double* Y, const double* theta, double* V_out,
                    double* resid_out) {
  if (!ctx || k < 1 || !Y || !theta) return fail(ctx, RBL_ERR_INVALID, "rbl_ritz_finish: bad arguments");
  if (!ctx->d_rv || !ctx->d_rw || ctx->ritz_k != k)
    return fail(ctx, RBL_ERR_STATE, "rbl_ritz_finish: no rbl_ritz_project of this k precedes it");
  return rbl_ritz_finish_cols(ctx, k, k, Y, theta, V_out, resid_out);
}

// The projected width kproj (rows of Y, padded to kpr) and the kept pairs k (columns of Y, padded
// to kp): with kproj == k every buffer and launch is rbl_ritz_finish's of before.
int rbl_ritz_finish_cols(rbl_ctx* ctx, int kproj, int k, const double* Y, const double* theta,
                         double* V_out, double* resid_out) {
  if (!ctx || k < 1 || kproj < k || !Y || !theta)
    return fail(ctx, RBL_ERR_INVALID, "rbl_ritz_finish_cols: bad arguments (needs 1 <= k <= kproj)");
  if (!ctx->d_rv || !ctx->d_rw || ctx->ritz_k != kproj)
    return fail(ctx, RBL_ERR_STATE, "rbl_ritz_finish_cols: no rbl_ritz_project of this kproj precedes it");
  HIPC(hipSetDevice(ctx->device));
  const int kpr = (kproj + 1) & ~1;
  const int kp = (k + 1) & ~1;
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  std::vector<double> yrm((size_t)kpr * kp, 0.0), th(kp, 0.0), res(kp, 0.0);
  for (int r = 0; r < kproj; ++r)
    for (int c = 0; c < k; ++c) yrm[(size_t)r * kp + c] = Y[(size_t)c * kproj + r];
  for (int c = 0; c < k; ++c) th[c] = theta[c];
  const int grid = resid_grid(ctx->nloc);
  DevBuf<double> dY, dTh, X, Z, part, dres;
  HIPC(dY.alloc((size_t)kpr * kp));
  HIPC(dTh.alloc(kp));
  HIPC(X.alloc((size_t)nl * kp));
  HIPC(Z.alloc((size_t)nl * kp));
  HIPC(part.alloc((size_t)grid * kp));
  HIPC(dres.alloc(kp));
  HIPC(hipMemcpyAsync(dY, yrm.data(), (size_t)kpr * kp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(hipMemcpyAsync(dTh, th.data(), kp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (ctx->nloc > 0) {
    StageScope t(ctx, RBL_STAGE_RITZ);
    // X = V Y, Z = W Y; resid_j^2 = sum_r (Z - X diag(theta))^2[r, j]
    CHK(tsmm_checked(ctx, run1(ctx->d_rv, kpr), dY, kp, pan1(X, kp), 1.0, 0.0, nullptr));
    CHK(tsmm_checked(ctx, run1(ctx->d_rw, kpr), dY, kp, pan1(Z, kp), 1.0, 0.0, nullptr));
    resid_partial(ctx->nloc, kp, Z, X, dTh, part, grid, ctx->stream);
    reduce_slab(part, grid, kp, dres, nullptr, ctx->stream);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(res.data(), dres, kp * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (V_out) {  // W is spent: its block takes the column-major copy of X
      rowmajor_to_colmajor(X, ctx->nloc, kp, ctx->d_rw, ctx->stream);
      HIPC(hipGetLastError());
      CHK(d2h_staged(ctx, V_out, ctx->d_rw, (size_t)ctx->nloc * k * sizeof(double)));
    }
  }
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  if (resid_out)
    for (int c = 0; c < k; ++c) resid_out[c] = std::sqrt(res[c]);
  ctx->d_rv.reset();
  ctx->d_rw.reset();
  ctx->ritz_k = 0;
  return RBL_OK;
}

int rbl_get_block(rbl_ctx* ctx, int j, double* Q_out) {
  if (!ctx || j < 1 || j > ctx->nblocks || !Q_out) return fail(ctx, RBL_ERR_INVALID, "rbl_get_block: bad block");
  HIPC(hipSetDevice(ctx->device));
  const int b = ctx->b;
  int st = 0;
  const double* src = ctx->basis_bits == 64 ? block_dev(ctx, j - 1, ctx->nblocks, &st) : nullptr;
  if (st) return fail(ctx, st, "rbl_get_block: H2D of a spilled block failed");
  if (ctx->basis_bits == 32) {  // fp32 slot, returned widened
    CHK(ensure_qm64(ctx));
    const float* s32 = block_dev32(ctx, j - 1, ctx->nblocks, &st);
    if (st) return fail(ctx, st, "rbl_get_block: H2D of a spilled block failed");
    cvt_f32_to_f64(s32, ctx->d_Qm64, ctx->nloc * b, ctx->stream);
    src = ctx->d_Qm64;
  }
  rowmajor_to_colmajor(src, ctx->nloc, b, ctx->d_T, ctx->stream);
  HIPC(hipMemcpyAsync(Q_out, ctx->d_T, ctx->nloc * b * sizeof(double), hipMemcpyDeviceToHost,
                      ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  return RBL_OK;
}

int rbl_num_blocks(rbl_ctx* ctx) { return ctx ? ctx->nblocks : 0; }

// ---- restarted variants (restarted.jl) -------------------------------------------------
int rbl_restart(rbl_ctx* ctx, int nblocks, const double* S) {
  if (ctx) ctx->cloc_step = 0;  // the basis changes outside the step
  if (ctx) shadow_written(ctx, 0);
  if (ctx) ctx->arrow_kb = 0;
  if (!ctx || !S || nblocks < 1 || nblocks > ctx->nblocks)
    return fail(ctx, RBL_ERR_INVALID, "rbl_restart: bad arguments");
  if (!ctx->d_basis) return fail(ctx, RBL_ERR_STATE, "rbl_restart: needs an fp64 run (rbl_start)");
  if (spilled(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_restart: needs an HBM-resident basis");
  HIPC(hipSetDevice(ctx->device));
  const int b = ctx->b;
  CHK(basis_combine(ctx, nblocks, b, S, ctx->d_T));
  HIPC(hipMemcpyAsync(slotp(ctx, 0), ctx->d_T, ctx->nloc * b * sizeof(double),
                      hipMemcpyDeviceToDevice, ctx->stream));
  HIPC(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  ctx->nblocks = 1;
  ctx->fetched = 1;
  return RBL_OK;
}

// ---- thick restart ---------------------------------------------------------------------
// Every refusal comes before any change: the basis, the block count and a pending arrow stay as
// they were.
int rbl_thick_restart(rbl_ctx* ctx, int nblocks, int keep_blocks, const double* S, const double* W) {
  if (!ctx) return RBL_ERR_INVALID;
  const int m = nblocks, kb = keep_blocks;
  if (!S || !W) return fail(ctx, RBL_ERR_INVALID, "rbl_thick_restart: S or W is NULL");
  if (ctx->nranks > 1)
    return fail(ctx, RBL_ERR_INVALID, "rbl_thick_restart: one rank only (nranks > 1 is not supported)");
  if (ctx->d_basis32)
    return fail(ctx, RBL_ERR_STATE, "rbl_thick_restart: the fp64 basis only (the current run has basis_bits = 32)");
  if (!ctx->d_basis || ctx->nblocks < 1)
    return fail(ctx, RBL_ERR_STATE, "rbl_thick_restart: needs an fp64 run (rbl_start)");
  if (spilled(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_thick_restart: needs an HBM-resident basis");
  if (ctx->fetched < ctx->nblocks)
    return fail(ctx, RBL_ERR_STATE, "rbl_thick_restart: rbl_fetch the asynchronous steps first");
  if (m < 1 || m + 1 != ctx->nblocks)
    return fail(ctx, RBL_ERR_STATE, "rbl_thick_restart: nblocks + 1 must equal the current block count (" +
                                        std::to_string(ctx->nblocks) + ")");
  if (kb < 1 || kb >= m)
    return fail(ctx, RBL_ERR_INVALID, "rbl_thick_restart: keep_blocks must be in [1, nblocks)");
  const int b = ctx->b;
  const int64_t p = (int64_t)kb * b, mb = (int64_t)m * b;
  if (p > RBL_COMPRESS_MAX_COLS)
    return fail(ctx, RBL_ERR_INVALID, "rbl_thick_restart: keep_blocks * b = " + std::to_string(p) +
                                          " exceeds RBL_COMPRESS_MAX_COLS = " +
                                          std::to_string(RBL_COMPRESS_MAX_COLS));
  for (int64_t e = 0; e < mb * p; ++e)
    if (!std::isfinite(S[e])) return fail(ctx, RBL_ERR_INVALID, "rbl_thick_restart: S has a non-finite entry");
  for (int64_t e = 0; e < (int64_t)b * p; ++e)
    if (!std::isfinite(W[e])) return fail(ctx, RBL_ERR_INVALID, "rbl_thick_restart: W has a non-finite entry");
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  // S column-major (m b) x p -> row-major; W column-major b x p is W^T row-major p x b as it lies
  std::vector<double> Sr((size_t)(mb * p));
  for (int64_t c = 0; c < p; ++c)
    for (int64_t r = 0; r < mb; ++r) Sr[(size_t)(r * p + c)] = S[r + c * mb];
  if (ctx->tr_S_cap < Sr.size()) {
    ctx->d_tr_S.reset();
    ctx->tr_S_cap = 0;
    HIPC(ctx->d_tr_S.alloc(Sr.size()));
    ctx->tr_S_cap = Sr.size();
  }
  if (ctx->arrow_W_cap < (size_t)(p * b)) {
    ctx->d_arrow_W.reset();
    ctx->arrow_W_cap = 0;
    HIPC(ctx->d_arrow_W.alloc((size_t)(p * b)));
    ctx->arrow_W_cap = (size_t)(p * b);
  }
  HIPC(hipMemcpy(ctx->d_tr_S, Sr.data(), Sr.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->d_arrow_W, W, (size_t)(p * b) * sizeof(double), hipMemcpyHostToDevice));
  {
    StageScope t(ctx, RBL_STAGE_RITZ);
    PanelRun X;
    X.base = slotp(ctx, 0);
    X.stride = ctx->slot;
    X.count = m;
    X.w = b;
    if (!basis_compress(ctx->nloc, X, ctx->d_tr_S, (int)p, ctx->stream))
      return fail(ctx, RBL_ERR_INVALID, "internal: basis_compress does not serve this shape");
    HIPC(hipGetLastError());
    // slot kb <- Q_{m+1} (kb < m: the compression has read slot kb and never touches slot m)
    HIPC(hipMemcpyAsync(slotp(ctx, kb), slotp(ctx, m), ctx->slot * sizeof(double),
                        hipMemcpyDeviceToDevice, ctx->stream));
  }
  HIPC(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  ctx->cloc_step = 0;  // the basis changes outside the step
  ctx->cloc_final = false;
  shadow_written(ctx, 0);  // the compression rewrote slots 0 .. kb
  ctx->nblocks = kb + 1;
  ctx->fetched = kb + 1;
  ctx->arrow_kb = kb;
  return RBL_OK;
}

// Diagnostics: hipEvent time per pass of the in-place compression of a run of m synthetic
// rows x b blocks to keep_blocks blocks, and of the route without it — ceil(p / 64) out-of-place
// tsmm launches, each re-reading the whole run, into a rows x 64 scratch block.  The blocks, S and
// the scratch are allocated and zeroed for the call.
int rbl_bench_compress_pass(rbl_ctx* ctx, int64_t rows, int b, int m, int keep_blocks, int reps,
                            double* inplace_ms, double* sliced_ms) {
  if (!ctx || rows < 1 || b < 1 || b > RBL_MAX_BLOCK || m < 2 || keep_blocks < 1 || keep_blocks >= m ||
      (int64_t)keep_blocks * b > RBL_COMPRESS_MAX_COLS || reps < 1 || !inplace_ms || !sliced_ms)
    return fail(ctx, RBL_ERR_INVALID, "rbl_bench_compress_pass: bad arguments");
  HIPC(hipSetDevice(ctx->device));
  const int p = keep_blocks * b;
  const int64_t slot = rows * b;
  DevBuf<double> x, s, y;
  const std::pair<DevBuf<double>*, size_t> bufs[] = {{&x, (size_t)slot * m},
                                             {&s, (size_t)m * b * p},
                                             {&y, (size_t)rows * 64}};
  for (const auto& q : bufs) {
    HIPC(q.first->alloc(q.second));
    HIPC(hipMemsetAsync(*q.first, 0, q.second * sizeof(double), ctx->stream));
  }
  PanelRun X;
  X.base = x;
  X.stride = slot;
  X.count = m;
  X.w = b;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  int st = RBL_OK;
  auto inplace = [&] {
    if (!basis_compress(rows, X, s, p, ctx->stream)) st = RBL_ERR_INVALID;
  };
  auto sliced = [&] {
    for (int c0 = 0; c0 < p; c0 += 64)
      tsmm(rows, X, s + c0, p, pan1(y, std::min(64, p - c0)), 1.0, 0.0, nullptr, ctx->stream);
  };
  auto timed = [&](auto&& fn, double* out) {
    fn();  // warm-up
    if (hipEventRecord(e0, ctx->stream) != hipSuccess) st = RBL_ERR_HIP;
    for (int q = 0; q < reps; ++q) fn();
    if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) st = RBL_ERR_HIP;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) st = RBL_ERR_HIP;
    *out = (double)ms / reps;
  };
  timed(inplace, inplace_ms);
  timed(sliced, sliced_ms);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st != RBL_OK) return fail(ctx, st, "rbl_bench_compress_pass: a HIP call failed");
  return RBL_OK;
}

int rbl_lock(rbl_ctx* ctx, int nblocks, int nvec, const double* S) {
  if (ctx) ctx->cloc_step = 0;  // the basis changes outside the step
  if (ctx) shadow_written(ctx, 0);  // (a restart follows a lock: nothing of the shadow is kept)
  if (!ctx || !S || nblocks < 1 || nblocks > ctx->nblocks || nvec < 0)
    return fail(ctx, RBL_ERR_INVALID, "rbl_lock: bad arguments");
  if (!ctx->d_basis) return fail(ctx, RBL_ERR_STATE, "rbl_lock: needs an fp64 run (rbl_start)");
  if (spilled(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_lock: needs an HBM-resident basis");
  if (nvec == 0) return RBL_OK;
  HIPC(hipSetDevice(ctx->device));
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  if (ctx->nlock + nvec > ctx->lock_cap) {
    const int cap = std::max(2 * ctx->lock_cap, ctx->nlock + nvec);
    DevBuf<double> d;
    HIPC(d.alloc((size_t)cap * nl));
    if (ctx->nlock)
      HIPC(hipMemcpyAsync(d, ctx->d_lock, (size_t)ctx->nlock * nl * sizeof(double),
                          hipMemcpyDeviceToDevice, ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    ctx->d_lock = std::move(d);
    ctx->lock_cap = cap;
  }
  const int64_t rows = (int64_t)nblocks * ctx->b;
  for (int v = 0; v < nvec; ++v)
    CHK(basis_combine(ctx, nblocks, 1, S + v * rows, ctx->d_lock + (int64_t)(ctx->nlock + v) * nl));
  ctx->nlock += nvec;
  return RBL_OK;
}

int rbl_num_locked(rbl_ctx* ctx) { return ctx ? ctx->nlock : 0; }

int rbl_get_locked(rbl_ctx* ctx, double* V_out) {
  if (!ctx || !V_out) return fail(ctx, RBL_ERR_INVALID, "rbl_get_locked: bad arguments");
  if (ctx->nlock == 0) return RBL_OK;
  HIPC(hipSetDevice(ctx->device));
  const int64_t nl = std::max<int64_t>(ctx->nloc, 1);
  for (int j = 0; j < ctx->nlock; ++j)  // vector j is a contiguous column of length n_local
    HIPC(hipMemcpy(V_out + (int64_t)j * ctx->nloc, ctx->d_lock + (int64_t)j * nl,
                   ctx->nloc * sizeof(double), hipMemcpyDeviceToHost));
  return RBL_OK;
}

int rbl_reorth_last(rbl_ctx* ctx, int nblocks, int flags) {
  if (ctx) ctx->cloc_step = 0;  // the basis changes outside the step
  if (!ctx || nblocks < 1 || nblocks > ctx->nblocks)
    return fail(ctx, RBL_ERR_INVALID, "rbl_reorth_last: bad arguments");
  if (!ctx->d_basis) return fail(ctx, RBL_ERR_STATE, "rbl_reorth_last: needs an fp64 run");
  if (spilled(ctx)) return fail(ctx, RBL_ERR_STATE, "rbl_reorth_last: needs an HBM-resident basis");
  HIPC(hipSetDevice(ctx->device));
  CHK(reorth_pair(ctx, nblocks, flags));
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  return RBL_OK;
}

int rbl_num_stages(void) { return RBL_NUM_STAGES; }
const char* rbl_stage_name(int stage) {
  return (stage >= 0 && stage < RBL_NUM_STAGES) ? kStageNames[stage] : "";
}
int rbl_timers(rbl_ctx* ctx, double* ms, int nstages) {
  if (!ctx || !ms) return RBL_ERR_INVALID;
  for (int s = 0; s < nstages && s < RBL_NUM_STAGES; ++s) ms[s] = ctx->stage_ms[s];
  return RBL_OK;
}
int rbl_allgather_host(rbl_ctx* ctx, const int64_t* mine, int64_t* all, int n) {
  if (!ctx || n < 0 || (n > 0 && (!mine || !all))) return fail(ctx, RBL_ERR_INVALID, "rbl_allgather_host: bad arguments");
  if (n == 0) return RBL_OK;
  HIPC(hipSetDevice(ctx->device));
  if (ctx->nranks == 1) {
    memcpy(all, mine, (size_t)n * sizeof(int64_t));
    return RBL_OK;
  }
  COMMC(ctx->comm->allgather_host(mine, all, (size_t)n, ctx->stream, &ctx->err));
  return RBL_OK;
}

int rbl_comm_stats(rbl_ctx* ctx, int64_t* out, int nstats, int reset) {
  if (!ctx || nstats < 0 || (nstats > 0 && !out)) return RBL_ERR_INVALID;
  for (int i = 0; i < nstats && i < RBL_COMM_NSTATS; ++i) out[i] = ctx->comm_stats[i];
  // the halo plan of the matrix held (not counters: reset leaves them)
  if (nstats > RBL_COMM_HALO_PUSH) out[RBL_COMM_HALO_PUSH] = ctx->push ? 1 : 0;
  if (nstats > RBL_COMM_PUSH_ROWS) out[RBL_COMM_PUSH_ROWS] = ctx->push_pred_rows;
  if (nstats > RBL_COMM_PULL_ROWS) out[RBL_COMM_PULL_ROWS] = ctx->pull_pred_rows;
  // the time in the collectives: host wall time in the calls, hipEvent spans on their streams
  const int64_t tm[4] = {ctx->comm_host_ns[0], ctx->comm_host_ns[1],
                         (int64_t)(ctx->comm_dev_ms[0] * 1e6), (int64_t)(ctx->comm_dev_ms[1] * 1e6)};
  for (int i = RBL_COMM_PULL_ROWS + 1; i < nstats; ++i)
    out[i] = i <= RBL_COMM_EXCHANGE_DEV_NS ? tm[i - RBL_COMM_ALLREDUCE_HOST_NS] : 0;
  if (reset) {
    for (int64_t& v : ctx->comm_stats) v = 0;
    ctx->comm_host_ns[0] = ctx->comm_host_ns[1] = 0;
    ctx->comm_dev_ms[0] = ctx->comm_dev_ms[1] = 0.0;
  }
  return RBL_OK;
}

int rbl_path_stats(rbl_ctx* ctx, int64_t* out, int nstats, int reset) {
  if (!ctx || nstats < 0 || (nstats > 0 && !out)) return RBL_ERR_INVALID;
  // the fp32-update gate counts on the device (k_upd32_gate): read back behind the stream
  if (ctx->d_upd32) {
    int cnt[4] = {0, 0, 0, 0};
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(hipMemcpy(cnt, ctx->d_upd32 + 2, sizeof(cnt), hipMemcpyDeviceToHost));
    ctx->path_stats[RBL_PATH_UPD32_TAKEN] = cnt[0];
    ctx->path_stats[RBL_PATH_UPD32_REFUSED] = cnt[1];
    ctx->path_stats[RBL_PATH_UPD32_SHADOW_READ] = cnt[2];
    ctx->path_stats[RBL_PATH_UPD32_SHADOW_CONV] = cnt[3];
    if (reset) HIPC(hipMemset(ctx->d_upd32 + 2, 0, sizeof(cnt)));
  }
  ctx->path_stats[RBL_PATH_UPD32_SHADOW_BYTES] = (int64_t)ctx->shadow_bytes;  // the plan's, not a count
  for (int i = 0; i < nstats; ++i) out[i] = i < RBL_PATH_NSTATS ? ctx->path_stats[i] : 0;
  if (reset)
    for (int64_t& v : ctx->path_stats) v = 0;
  return RBL_OK;
}

int rbl_shadow_valid(rbl_ctx* ctx) { return ctx && ctx->d_shadow ? ctx->shadow_valid : 0; }

int rbl_get_shadow_block(rbl_ctx* ctx, int j, float* out) {
  if (!ctx || !out || !ctx->d_shadow || j < 1 || j > ctx->shadow_valid)
    return fail(ctx, RBL_ERR_INVALID, "rbl_get_shadow_block: no valid shadow of that block");
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  std::vector<float> slot((size_t)ctx->shadow_slot);
  HIPC(hipMemcpy(slot.data(), ctx->d_shadow + (int64_t)(j - 1) * ctx->shadow_slot,
                 slot.size() * sizeof(float), hipMemcpyDeviceToHost));
  shadow_block_rowmajor(slot.data(), ctx->nloc, out);
  return RBL_OK;
}

int rbl_upd32_gate_values(rbl_ctx* ctx, double* out, int n) {
  if (!ctx || n < 0 || (n > 0 && !out)) return RBL_ERR_INVALID;
  for (int i = 0; i < n; ++i) out[i] = 0.0;
  if (!ctx->d_upd32_g || n == 0) return RBL_OK;
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  HIPC(hipMemcpy(out, ctx->d_upd32_g, (size_t)std::min(n, kUpd32Log) * sizeof(double), hipMemcpyDeviceToHost));
  return RBL_OK;
}

int rbl_reset_timers(rbl_ctx* ctx) {
  if (!ctx) return RBL_ERR_INVALID;
  for (double& v : ctx->stage_ms) v = 0.0;
  return RBL_OK;
}
int rbl_synchronize(rbl_ctx* ctx) {
  if (!ctx) return RBL_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  harvest_timers(ctx);
  return RBL_OK;
}

}  // extern "C"
