/*
 * rbl_hip.h — C-ABI of librbl_hip.so, the MI355X (gfx950) Randomized Block Lanczos
 * inner loop.  Plain pointers and sizes only; no torch / HIP types cross this boundary.
 *
 * The reference (Iasonaspg/GPU-Randomized-Block-Lanczos) has no FFI layer: its "API" is
 * the Julia function pair RBL(A,k,b) (Julia/RBL.jl:119) / RBL_gpu(A,k,b)
 * (Julia/RBL_gpu.jl:205).  Its only native-call convention is the ccall into LAPACK at
 * Julia/common.jl:32-34 (ILP64 Ref{Int64} scalars, Ptr{Float64} column-major buffers).
 * This header follows that convention: int64 sizes, column-major dense buffers at the
 * boundary, caller-allocated outputs, every pointer borrowed only for the call.
 *
 * Each entry point below names the reference code it replaces.  The host loop that
 * replaces Julia/RBL_gpu.jl:162-194 (T_j assembly, dsbev, sort, convergence test —
 * Julia/common.jl:9-65) stays on the CPU and calls rbl_step() once per block step.
 *
 * Status codes: 0 ok, <0 error (rbl_last_error() has text), >0 warning.
 * Threading: one context per caller, not re-entrant; every entry point re-binds its
 * device, so callers may migrate between OS threads (Julia tasks).
 */
#ifndef RBL_HIP_H
#define RBL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: RBL_OPT_SPMM_KERNEL takes the kernel ids of rbl_spmm_kernel_for (5 band tiles, 6 segmented
 *    gather; version 1 took 4 / 5 for them) and rbl_create_shm was added.  A caller built
 *    against version 1 should check rbl_abi_version() before passing kernel ids. */
#define RBL_ABI_VERSION 2
/* Largest Krylov block size b (RBL_gpu(A, k, b) takes any b, RBL_gpu.jl:205; the reference's
 * scripts use b <= 8, the north star b = 32).  The MFMA fast paths cover b in {16, 32}. */
#define RBL_MAX_BLOCK 512

#define RBL_OK                  0
#define RBL_WARN_NOT_CONVERGED  1   /* host-side status for the P6 case */
#define RBL_WARN_QR_SHIFTED     2   /* rank-deficient block: shifted CholQR3 was used      */
#define RBL_ERR_INVALID        -1   /* bad argument / unsupported option                   */
#define RBL_ERR_HIP            -2   /* HIP runtime failure                                 */
#define RBL_ERR_OOM            -3   /* device allocation failed                            */
#define RBL_ERR_RCCL           -4   /* RCCL failure                                        */
#define RBL_ERR_STATE          -5   /* call out of order (e.g. step before start)          */
#define RBL_ERR_NUMERIC        -6   /* QR breakdown that the fallback could not repair     */

/* Timer stages; names match the reference's TimerOutputs labels (Julia/RBL_gpu.jl:152-187,219). */
#define RBL_STAGE_AQ          0   /* "AQ"            RBL_gpu.jl:152,176  SpMM + fused 3-term term */
#define RBL_STAGE_3TERM       1   /* "3-term"        RBL_gpu.jl:153-154,177-179                  */
#define RBL_STAGE_QR          2   /* "qr"            RBL_gpu.jl:155,180-184                      */
#define RBL_STAGE_PART_REORTH 3   /* "part reorth"   RBL_gpu.jl:165                               */
#define RBL_STAGE_LOC_REORTH  4   /* "loc reorth"    RBL_gpu.jl:167                               */
#define RBL_STAGE_RITZ        5   /* "Ritz vectors"  RBL_gpu.jl:219                               */
#define RBL_STAGE_COMM        6   /* halo exchange + all-reduce (no reference equivalent)         */
#define RBL_STAGE_SPILL_WAIT  7   /* "spill wait": host spill, the step's QR waiting for the D2H
                                   * copy-out of a finished block that shares its working slot  */
#define RBL_NUM_STAGES        8

/* Options for rbl_set_option(). */
#define RBL_OPT_TIMERS        0   /* 1: record per-stage hipEvents (adds event records);        */
                                  /*    2: only the "AQ" and "part reorth" stages (the kernels  */
                                  /*    the bench prices against their rooflines)               */
#define RBL_OPT_REORTH_ORDER  1   /* 0: block-CGS (batched, default); 1: ascending-j block MGS  */
                                  /*    exactly as RBL.jl:30-48 / RBL_gpu.jl:65-67               */
#define RBL_OPT_DEVICE_BLOCKS 3   /* Krylov blocks kept in HBM (the reference's hybrid buffer,
                                   * RBL_GPU.jl:24-27, 59-81, 95-132): 0 = all (default); -1 =
                                   * as many as fit in 80 % of free HBM (gpu_buffer_size);
                                   * G >= 3 = G slots: blocks 0..G-3 resident, the two newest
                                   * in two working slots, every older block in pinned host
                                   * memory, streamed back over PCIe for partial reorth and
                                   * Ritz.  fp64 or fp32 basis (the reference's buffer is typed
                                   * FLOAT, RBL_gpu.jl:59-81); set before rbl_start.            */
#define RBL_OPT_SPMM_KERNEL   2   /* 0: auto; otherwise the kernel id rbl_spmm_kernel_for reports:
                                   * 1 global-gather CSR; 2 LDS-window CSR (DPP); 3 LDS-densified
                                   * band on fp64 MFMA; 5 band-tile format (CSR densified once
                                   * into MFMA operand order, b in {16, 32}, |c - r| <= 64);
                                   * 6 segmented gather (power-law rows split / packed, b in
                                   * {16, 32}); 7 column panels (CSR rows in blocks of 256 / 512,
                                   * Q staged through LDS in 256-row panels of the columns a block
                                   * touches, b = 32; the default where every staged Q row is
                                   * read >= 4 times, i.e. bands wider than the band tiles' 64).
                                   * Each falls back 5 -> 3 -> 2 -> 1 (7 -> 1) when the matrix
                                   * does not fit the kernel's limits.  4 (dense panels) follows
                                   * from rbl_set_matrix_dense and is rejected here.  With a
                                   * rectangular B (rbl_set_matrix_normal) every value falls back
                                   * to 8, the rectangular gather pair.                        */
#define RBL_OPT_SPLIT_HALO    4   /* several ranks, band-tile SpMM: 1 (default) the kernel reads
                                   * the own rows from the block and the halo buffer holds only
                                   * the neighbours' rows; 0 the own block is copied into the
                                   * halo buffer every step (same results, bit for bit)         */
#define RBL_OPT_KEEP_CSR      5   /* 1 (default): the device CSR stays beside any SpMM format
                                   * built from it; 0: once the band tiles are built the CSR
                                   * (values, column ids, band positions, gather tables) is
                                   * released — 12 B per nonzero of HBM for the Krylov basis
                                   * (n = 5e7: 60 GB).  Then only b in {16, 32} can run and
                                   * rbl_get_matrix_csr fails.  Set before the matrix.          */
#define RBL_OPT_FUSE          6   /* pass fusions of the memory-bound b x b stages (b in {16, 32},
                                   * fp64 basis; default 7, all on):
                                   * bit 0: CholQR2 in 3 passes over the block instead of 4 (Q1
                                   *   recomputed, never stored) — bit for bit the same results;
                                   * bit 1: the next step's local-reorth Gram Q_i^T Q_{i+1} formed
                                   *   while the QR writes Q_{i+1} (used when that step runs no
                                   *   partial reorth), and Q_{i-1}^T Q_i by the last partial-
                                   *   reorth update — same results to rounding (1e-12);
                                   * bit 2: the local-reorth update Q_i -= Q_{i-1} C applied by
                                   *   the band-tile SpMM as it stages Q_i's rows (b = 32) — same
                                   *   results to rounding.  Works on several ranks: each rank
                                   *   corrects its first and last H rows (the rows its
                                   *   neighbours receive) before the halo exchange.  The
                                   *   several-rank form is tested with in-process ranks on one
                                   *   GPU; it has no run on several GPUs yet.               */

#define RBL_OPT_HALO_OVERLAP  7   /* several ranks, unbanded A (the segmented gather, whose halo is
                                   * most of Q_i): 1 (default) the halo exchange runs on a side
                                   * stream while the SpMM multiplies the own-column part of
                                   * each row, the halo-column part after it lands; 0 the same
                                   * two parts after the exchange (same results, bit for bit) */

#define RBL_OPT_RELABEL       8   /* 1: the next rbl_gen_matrix_rmat stores P A P^T for a seeded
                                   * permutation P (a Feistel bijection of the vertex ids): R-MAT's
                                   * hubs (its low ids) spread over the row range, so an
                                   * nnz-balanced row split gives every rank a like share of hub
                                   * and tail rows and of the halo it sends.  Eigenvalues are A's;
                                   * the device start block (omega NULL) draws row perm(v) from
                                   * v's id, so the run is the plain run permuted; rbl_row_ids gives
                                   * each local row's original id (a caller's omega and V rows are
                                   * in that order).  0 (default): A as drawn.                  */

#define RBL_OPT_HALO_PUSH     9   /* several ranks, unbanded A (the indexed halo of the segmented
                                   * gather), read when the matrix is set: each off-rank product
                                   * A[r,c] Q[c] is formed on the rank of the endpoint with the
                                   * larger (row degree, smaller id) — pulled Q[c] when that is c,
                                   * else computed by c's owner and its partial row pushed — so
                                   * the high-degree rows every rank references stay home and
                                   * only their partial rows move.  Needs A structurally
                                   * symmetric (checked from per-pair entry counts).  2 (default)
                                   * when its setup predicts fewer moved rows than pulling every
                                   * referenced row (< 0.85x); 1 always; 0 never.  Results differ
                                   * from the pull-all halo only in the order of each row's sum. */

#define RBL_OPT_CLOC_DERIVE   10  /* 1 (default): the local-reorth coefficient Q_{i-1}^T Q_i is
                                   * derived from sums the step forms anyway instead of a Gram
                                   * of its own.  The 3-term pass U' = U - Q_i A_i also forms
                                   * M = Q_i^T U' from the rows it holds, and CholQR's factors
                                   * give Q_i^T Q_{i+1} = M R1^-1 R2^-1 (R3^-1), so the QR's last
                                   * pass no longer reads Q_i.  On a step with a block-CGS partial
                                   * reorth (b = 32) the coefficient after it is G - Cm^T Ci with
                                   * G the one before it and [Ci | Cm] = W^T [Q_i | Q_{i-1}], the
                                   * reorth's own coefficients; the term Cm^T (W^T W - I) Ci is
                                   * dropped.  Where U' is graded (decided on the device from
                                   * R1: the derived value's error grows with cond(U')) or the
                                   * Cholesky was shifted, the QR's last pass forms the Gram as
                                   * before.  Same results to rounding (1e-12).  Needs the fp64
                                   * basis, b in {16, 32}, RBL_OPT_FUSE bits 0 and 1,
                                   * RBL_OPT_REORTH_ORDER 0 and a basis held whole in HBM (on
                                   * several ranks: RBL_OPT_DEVICE_BLOCKS 0); not used on
                                   * filtered steps or the arrow step after a thick restart.
                                   * 0, or any of these unmet: the routes of RBL_OPT_FUSE bit 1. */

#define RBL_OPT_UPD32         11  /* the partial-reorth update [Q_i | Q_{i-1}] -= W C with W C
                                   * formed on fp32 MFMA (W and C rounded to fp32, fp32 sums, the
                                   * subtraction in fp64) where C = W^T [Q_i | Q_{i-1}] is rounding
                                   * residue.  1 (default): decided per step on the device from the
                                   * all-reduced C, g = max_c |C_c|_2 sqrt(K) 2^-24 / eps <= 1/2
                                   * (the fp32 rounding of W C then stays below the fp64 rounding of
                                   * the subtraction; every rank decides alike); otherwise the fp64
                                   * update as before.  0: always fp64.  2: always fp32, for tests
                                   * and probes only: it does NOT preserve results when C is not
                                   * small.  Applies where the update runs plain: fp64 basis,
                                   * b = 32, RBL_OPT_REORTH_ORDER 0, all of W in HBM, the
                                   * RBL_OPT_CLOC_DERIVE route of that step, no locked vectors;
                                   * everything else keeps the fp64 update.  Counted in
                                   * rbl_path_stats (RBL_PATH_UPD32_TAKEN / _REFUSED). */
#define RBL_OPT_UPD32_SHADOW  12  /* 1 (default): the fp32 update of RBL_OPT_UPD32 reads W from an
                                   * fp32 shadow of the basis, max_blocks - 2 slots of n_local x 32
                                   * floats beside it: a block never changes once it is part of W,
                                   * so (float)w is formed once — by the update that first meets
                                   * the block, which stores what it rounds — and every later update
                                   * fetches 4 bytes per entry instead of 8.  Results do not change
                                   * by a bit.  Read by rbl_start when it plans a run: the shadow is
                                   * allocated for an fp64 basis at b = 32 with RBL_OPT_UPD32 != 0
                                   * and every block in HBM, when it fits beside the basis
                                   * (rbl_plan_shadow_fits), and kept while the plan is reused.  0, or
                                   * any of these unmet, or the allocation failing: the update reads
                                   * the fp64 basis as before.  RBL_PATH_UPD32_SHADOW_* count it. */

typedef struct rbl_ctx rbl_ctx;

int rbl_abi_version(void);
/* How this copy of the library was built: RBL_BUILD_VARIANTS set when it was compiled with
 * -DRBL_VARIANTS (tools/build_variant.sh: the measured-and-rejected kernel variants and their
 * A/B switches, for diagnostics only; the product build leaves them out). */
#define RBL_BUILD_VARIANTS 1
int rbl_build_flags(void);

/* ---- context ------------------------------------------------------------------------
 * Replaces the implicit CUDA.jl device state of RBL_gpu.jl:1-6. */
int rbl_create(rbl_ctx** ctx, int device);
/* One rank of a row-partitioned multi-GPU job (one process per GPU).  `unique_id` is the
 * 128-byte RCCL id produced by rbl_get_unique_id() on rank 0 and broadcast by the host. */
int rbl_get_unique_id(uint8_t unique_id[128]);
/* Self-test of the RCCL transport on one device: a one-rank communicator (ncclCommInitRank)
 * runs the three collective shapes of a row-partitioned step — in-place all-reduce, host
 * all-gather, grouped send/recv — on device buffers and checks them.  msg (optional) gets a
 * one-line verdict.  RCCL refuses two ranks on one device, so a 1-GPU box can test no more. */
int rbl_comm_selftest(int device, char* msg, int msg_len);
int rbl_create_dist(rbl_ctx** ctx, int device, int nranks, int rank, const uint8_t unique_id[128]);
/* In-process rank group: `nranks` contexts in ONE process, each driven by its own host thread
 * (several may share a GPU).  Same multi-rank code path as rbl_create_dist with the RCCL
 * transport replaced by host-staged copies; used to exercise partitioning, halos and the
 * distributed Grams on a single-GPU machine.  The group is reference-counted: release it
 * with rbl_local_group_free whenever convenient (contexts keep it alive). */
typedef struct rbl_group rbl_group;
int rbl_local_group_create(rbl_group** group, int nranks);
int rbl_local_group_free(rbl_group* group);
int rbl_create_local(rbl_ctx** ctx, int device, rbl_group* group, int rank);
/* One rank of a process-per-rank job whose collectives go through a POSIX shared-memory
 * segment (host-staged, pinned) instead of RCCL: the production orchestration — one process
 * and one HIP context per rank, rendezvous, setup collectives, the side-stream halo exchange —
 * with ranks that may share one GPU (RCCL refuses that).  Every rank passes the same `path`
 * (e.g. "/dev/shm/rbl_<nonce>", unique per job); rank 0 creates it, the others wait for it,
 * and it is unlinked once all ranks have mapped it.  A rank that exits or stalls past
 * RBL_SHM_TIMEOUT_S seconds (default 120) makes its peers' calls fail with RBL_ERR_RCCL.
 * Transport name "shm" (rbl_comm_info). */
int rbl_create_shm(rbl_ctx** ctx, int device, int nranks, int rank, const char* path);
int rbl_free(rbl_ctx* ctx);
const char* rbl_last_error(const rbl_ctx* ctx);
/* Ranks as the transport itself counts them (RCCL: ncclCommCount; in-process group: its size;
 * one rank: 1, transport "none"), this context's rank, and the transport's name. */
int rbl_comm_info(rbl_ctx* ctx, int* nranks, int* rank, char* transport, int transport_len);
/* The RCCL library every RCCL-transport context calls: ROCm's own, opened by path
 * (/opt/rocm/lib/librccl.so.1, or $RBL_RCCL_LIB) with a private symbol scope, whatever else
 * the process loaded first (torch bundles another RCCL with the same soname).  version gets
 * ncclGetVersion's code (22707 = 2.27.7); path (optional) the file it was loaded from, or the
 * loader's error.  No GPU call: safe before any context exists. */
int rbl_rccl_version(int* version, char* path, int path_len);
int rbl_set_option(rbl_ctx* ctx, int option, int64_t value);
/* Free and total HBM of the context's device (hipMemGetInfo): what a caller checks before it
 * sizes a run (the reference sizes its buffer from CUDA.available_memory, RBL_gpu.jl:95-104). */
int rbl_device_memory(rbl_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes);

/* ---- matrix --------------------------------------------------------------------------
 * Replaces `Ag = adapt(CuArray, A)` (RBL_gpu.jl:209).  The arrays are read as A's rows (CSR).
 * A is symmetric, so the CSC arrays of Julia's SparseMatrixCSC{Float64,Int64} are the CSR
 * arrays of A; `index_base` 1 accepts them unchanged.  For an unsymmetric A (benchmark.jl:58)
 * pass the CSC arrays of A^T — its CSR arrays — so the device computes A Q as cuSPARSE does
 * (julia/RBL_hip.jl and rbl.Context.set_matrix both do).  With nranks > 1 every rank passes the whole matrix and keeps the rows
 * [row_begin,row_end) of the nnz-balanced partition (rbl_plan_row_partition). */
int rbl_set_matrix_csc(rbl_ctx* ctx, int64_t n, int64_t nnz, const int64_t* colptr,
                       const int64_t* rowval, const double* nzval, int index_base);
/* Local CSR rows [row_begin,row_end) of an n x n symmetric matrix, global column ids. */
int rbl_set_matrix_csr_rows(rbl_ctx* ctx, int64_t n, int64_t row_begin, int64_t row_end,
                            const int64_t* rowptr, const int64_t* colind, const double* val,
                            int index_base);
/* Dense symmetric A (RBL_gpu(A::Matrix{Float64}, k, b), RBL_gpu.jl:205; images.jl's B^T B):
 * the local rows [row_begin,row_end) as a column-major slice with leading dimension lda
 * (one rank: the whole n x n matrix, lda >= n — Julia's Matrix pointer as-is).  A * Q then
 * runs as a panel GEMM on fp64 MFMA with Q gathered to all n rows on every rank.
 * rbl_spmm_kernel_for reports 4; rbl_get_matrix_csr fails (RBL_ERR_STATE). */
int rbl_set_matrix_dense(rbl_ctx* ctx, int64_t n, int64_t row_begin, int64_t row_end,
                         const double* A, int64_t lda);
/* Device-side generator of the seeded symmetric "hash-window" matrix:
 * entry (r,c), |r-c| <= halfwidth, r != c, exists iff hash(seed,min,max) < density, with a
 * uniform(-1,1) value from the same hash; diagonal = uniform(-1,1) plus plant[l] at row
 * l*floor(n/nplant) for l < nplant.  Each rank generates only its own rows. */
/* Rectangular sparse B (nrows x ncols) for its k largest singular triplets (images.jl:20-33 runs
 * RBL_gpu(transpose(B)*B, k, 1) and recovers U = (B*V) ./ transpose(D)): the Krylov operator is
 * B^T B (ncols x ncols), applied as B^T (B Q) and never formed.
 *   layout 0: ptr / ind are B's CSR (ptr: nrows + 1, ind: column ids);
 *   layout 1: B's CSC (ptr: ncols + 1, ind: row ids) — Julia's SparseMatrixCSC as it is
 *             (index_base 1).  Passing B's CSR with layout 1 and the sizes swapped sets B^T.
 * Indices strictly ascending within each row (layout 0) / column (layout 1): sorted, no
 * duplicates.  The device holds both orientations (int32 ids, int64 row pointers: 2 x 12 B per
 * nonzero + (nrows + ncols + 2) x 8 B, and an nrows x b fp64 work block); the orientation not
 * passed is built on the device, every row ascending in the other index — the same arrays on
 * every run.  nrows, ncols < 2^31 and nnz < 2^31 - 1, else RBL_ERR_INVALID.
 * Afterwards: rbl_matrix_info reports n = ncols, rows [0, ncols), nnz_local = nnz; rbl_apply
 * computes B^T B X; rbl_start / rbl_step / rbl_ritz run on B^T B (eigenvalues sigma^2, Ritz
 * vectors = right singular vectors); rbl_spmm_kernel_for reports 8 for every b and
 * rbl_matrix_format 5; rbl_get_matrix_csr fails (RBL_ERR_STATE, as for a dense A);
 * RBL_OPT_KEEP_CSR has no effect and a forced RBL_OPT_SPMM_KERNEL falls back to kernel 8.
 * Limits: one rank only — on a context with nranks > 1 this returns RBL_ERR_INVALID before any
 * collective; the fp64 basis only — rbl_start with basis_bits = 32 returns RBL_ERR_INVALID. */
#define RBL_SPMM_KERNEL_RECT   8   /* rbl_spmm_kernel_for with a rectangular B */
#define RBL_MATRIX_FORMAT_RECT 5   /* rbl_matrix_format with a rectangular B   */
int rbl_set_matrix_normal(rbl_ctx* ctx, int64_t nrows, int64_t ncols, int64_t nnz,
                          const int64_t* ptr, const int64_t* ind, const double* val,
                          int index_base, int layout);
/* Shape of the rectangular B held (RBL_ERR_STATE when the matrix is of another kind). */
int rbl_rect_info(rbl_ctx* ctx, int64_t* nrows, int64_t* ncols, int64_t* nnz);
/* Download one orientation (trans 0: B's CSR, nrows + 1 pointers; 1: B^T's CSR, ncols + 1),
 * 0-based — test/inspection only. */
int rbl_get_matrix_rect(rbl_ctx* ctx, int trans, int64_t* rowptr, int32_t* colind, double* val);
/* One pass of the pair, host column-major blocks: trans 0: Y (nrows x b) = B X (ncols x b);
 * trans 1: Y (ncols x b) = B^T X (nrows x b).  Timed under "AQ" while RBL_OPT_TIMERS is set. */
int rbl_apply_rect(rbl_ctx* ctx, int trans, int b, const double* X, double* Y);
/* Left singular vectors U_out (nrows x k, column-major) = B V diag(1 / sigma) — images.jl:24,
 * `U = (B*V) ./ transpose(D)` — from V (ncols x k, column-major) and the k singular values:
 * pass 1 of the pair with the per-column scale in its epilogue.  k <= RBL_MAX_BLOCK.  With a
 * shift set (rbl_set_rect_shift) U_out = (B V - u (v^T V)) diag(1 / sigma) = C V diag(1 / sigma),
 * the shift subtracted before the scale. */
int rbl_left_vectors(rbl_ctx* ctx, int k, const double* V, const double* sigma, double* U_out);
/* Rank-one shift of the rectangular B held: C = B - u v^T (u: nrows entries, v: ncols entries,
 * both copied to the device; the caller's arrays are not kept).  PCA with implicit centring is
 * u = 1, v = the column means; centring on the other side, correspondence analysis
 * (B - r c^T / N) and the removal of a known singular pair are other choices of u, v.  C is
 * never formed: a block step applies
 *     t = Q^T v,   Y = B Q - u t^T,   s = Y^T u,   U = B^T Y - v s^T (- Q_{i-1} B_i^T)
 * — the two gather passes with  out[row][c] -= a[row] * w[c]  in their epilogues and two
 * reductions to b values each, all enqueued on the context's stream with no host
 * synchronisation; every sum has a fixed order (no atomics), so two runs give the same bits.
 * The operator is exactly C^T C for whatever u, v are stored (symmetric for any shift).
 * While a shift is set rbl_apply, rbl_start, rbl_step, rbl_step_async, the restarted entry
 * points and rbl_ritz_project run on C^T C and rbl_left_vectors returns C V diag(1 / sigma);
 * rbl_apply_rect stays the plain B / B^T.  Set it before rbl_start: a run in flight is waited
 * for, and its basis belongs to the operator it was built with.
 * Both NULL clears the shift (results are then bit for bit those of a context that never had
 * one); setting any matrix clears it too.  RBL_ERR_STATE without a rectangular matrix;
 * RBL_ERR_INVALID when exactly one pointer is NULL or an entry is not finite — the context and
 * an earlier shift stay as they were.  Limits as for the rectangular path: one rank, fp64 basis,
 * no filter.  Extra device memory: (nrows + ncols) x 8 B and under 8 workgroups per CU x b x 8 B. */
int rbl_set_rect_shift(rbl_ctx* ctx, const double* u, const double* v);
/* Download the shift set (u_out: nrows, v_out: ncols; either may be NULL) — test/inspection only.
 * RBL_ERR_STATE when no shift is set. */
int rbl_get_rect_shift(rbl_ctx* ctx, double* u_out, double* v_out);
/* One pass of the shifted pair, host column-major blocks as for rbl_apply_rect: trans 0:
 * Y (nrows x b) = C X = B X - u (v^T X);  trans 1: Y (ncols x b) = C^T X = B^T X - v (u^T X).
 * Without a shift it equals rbl_apply_rect bit for bit.  b <= RBL_MAX_BLOCK; timed under "AQ"
 * (the reduction included) while RBL_OPT_TIMERS is set. */
int rbl_apply_rect_shifted(rbl_ctx* ctx, int trans, int b, const double* X, double* Y);
/* Implicit kernel matrix over n points in d dimensions (X: n x d column-major, leading dimension
 * ldx >= n; copied, the caller's array is not kept):
 *     Op = diag(s) K diag(s) + nugget I,    K_ij = kappa(x_i, x_j),
 *   RBL_KERNEL_RBF      exp(-gamma |x - y|^2)
 *   RBL_KERNEL_LAPLACE  exp(-gamma |x - y|_2)
 *   RBL_KERNEL_POLY     (gamma x^T y + coef0)^degree
 * K is never formed: the device keeps the n x 4 ceil(d / 4) points and their squared norms, and
 * every product Op Q evaluates K tile by tile on fp64 MFMA (column chunks of 32 and 16; what is
 * left of any other width by a plain kernel), O(n^2 (d + b)) flops on O(n (d + b)) bytes.
 * Distances are taken in Gram form |x_i|^2 + |x_j|^2 - 2 x_i^T x_j, clamped at 0 and set to 0 on
 * the diagonal, so K_ii = 1 exactly for the two radial kernels (mean-centre the points first: the
 * cancellation grows with their norms); K is symmetric bit for bit.  Fixed summation order, no
 * atomics: two applications give the same bits.  gamma finite and > 0, coef0 finite, 1 <= degree
 * <= 8 (checked for every kind; coef0 and degree are used by RBL_KERNEL_POLY only), 1 <= d <=
 * RBL_KERNOP_MAX_DIM, X finite — else RBL_ERR_INVALID, the context unchanged.
 * Afterwards: rbl_matrix_info reports n, rows [0, n), nnz_local = n^2; rbl_apply, rbl_start /
 * rbl_step / rbl_ritz, the restarted and thick-restarted entry points, the Chebyshev filters,
 * series, moments and diagonal, and rbl_set_lowrank run on Op; rbl_spmm_kernel_for reports
 * RBL_SPMM_KERNEL_KERNOP for every b and rbl_matrix_format RBL_MATRIX_FORMAT_KERNOP;
 * rbl_get_matrix_csr fails (RBL_ERR_STATE).  Setting any matrix clears it, its scale and nugget.
 * Limits: one rank only — on a context with nranks > 1 this returns RBL_ERR_INVALID before any
 * collective; the fp64 basis only — rbl_start with basis_bits = 32 returns RBL_ERR_INVALID. */
#define RBL_KERNEL_RBF      0
#define RBL_KERNEL_LAPLACE  1
#define RBL_KERNEL_POLY     2
#define RBL_KERNOP_MAX_DIM  256
#define RBL_SPMM_KERNEL_KERNOP   9   /* rbl_spmm_kernel_for with a kernel matrix */
#define RBL_MATRIX_FORMAT_KERNOP 6   /* rbl_matrix_format with a kernel matrix   */
int rbl_set_matrix_kernel(rbl_ctx* ctx, int64_t n, int d, const double* X, int64_t ldx, int kind,
                          double gamma, double coef0, int degree);
/* The scale s (n entries, copied; NULL: all ones, nothing stored) and the nugget of the kernel
 * matrix held: s = deg^-1/2 gives the normalised affinity D^-1/2 K D^-1/2, the nugget K + tau I.
 * A run in flight is waited for.  (NULL, 0) returns to the bits of a context that never had them.
 * RBL_ERR_STATE without a kernel matrix; RBL_ERR_INVALID for a non-finite entry or nugget — the
 * context and an earlier scale stay as they were. */
int rbl_set_kernel_scale(rbl_ctx* ctx, const double* scale, double nugget);
/* What the kernel matrix held was set with (any pointer may be NULL); RBL_ERR_STATE without one. */
int rbl_kernel_info(rbl_ctx* ctx, int64_t* n, int* d, int* kind, double* gamma, double* coef0,
                    int* degree, int* has_scale, double* nugget);
/* Milliseconds per application of the kernel matrix held to a device-resident N(0,1) block of b
 * columns: one warm-up pass, then `reps` passes between two hipEvents.  RBL_ERR_STATE without one. */
int rbl_bench_kernel_pass(rbl_ctx* ctx, int b, int reps, double* ms);
/* Cross-kernel product of the kernel matrix held (points X, n x d; scale s) with m new points Z
 * (m x d, column-major, ldz >= m) — what every out-of-sample use of a kernel fit needs (kernel PCA's
 * transform, the Nystrom extension, a Gaussian process's mean and variance):
 *   trans = 0:  Y (m x b) = kappa(Z, X) diag(s) W,   W n x b  (ldw >= n, ldy >= m)
 *   trans = 1:  Y (n x b) = diag(s) kappa(X, Z) W,   W m x b  (ldw >= m, ldy >= n)
 * host column-major blocks like rbl_apply.  kappa(Z, X) is evaluated tile by tile on fp64 MFMA and
 * never stored; any 1 <= b <= RBL_MAX_BLOCK runs on MFMA (column chunks of 32 and 16, a narrower
 * last chunk zero-padded to 16).  The nugget never enters and there is no diagonal rule: where a row
 * of Z coincides with a row of X the entry is kappa of the Gram-form distance, within rounding of
 * kappa(0) and not exactly it.  The column range is split over rbl_kernel_cross_splits(rows of Y,
 * rows of W, d) workgroup columns, whose partials are added in ascending order by one thread per
 * output: no atomics, two calls give the same bits, and the bits do not depend on the device's CU
 * count.  Runs on the context's stream; extra device memory for the call only: the points of Z, the
 * two blocks and splits x rows x b doubles of partials.
 * RBL_ERR_STATE without a kernel matrix; RBL_ERR_INVALID for m < 1, b outside [1, RBL_MAX_BLOCK],
 * trans not 0 or 1, a NULL pointer, a leading dimension below its block's rows, or a non-finite
 * entry of Z or W — the context unchanged (a following rbl_apply gives the bits of one before). */
int rbl_kernel_cross(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int trans, int b,
                     const double* W, int64_t ldw, double* Y, int64_t ldy);
/* The number of splits S of the column range rbl_kernel_cross uses for a rows x cols product in d
 * dimensions — a function of the three numbers alone (no context, no device): the fewest splits with
 * ceil(rows / 64) S >= 512 workgroups, at most 64, each split at least 4 stages of 64 (d <= 16), 32
 * (d <= 64) or 16 column points; 1 when rows >= 32705.  RBL_ERR_INVALID for a bad argument. */
int rbl_kernel_cross_splits(int64_t rows, int64_t cols, int d);
/* Milliseconds per cross-kernel product of the matrix held with the m points Z against a
 * device-resident N(0,1) block of b columns (the device part of rbl_kernel_cross alone): one warm-up,
 * then `reps` products between two hipEvents.  splits = 0: the rule above; otherwise that many
 * (RBL_ERR_INVALID beyond 64 or the stages of the column range). */
int rbl_bench_kernel_cross(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int trans, int b,
                           int splits, int reps, double* ms);
/* The k nearest neighbours among the points X (n x d) of the kernel matrix held — the step that turns
 * points into a sparse k-nearest-neighbour graph for the sparse eigensolver:
 *   Z == NULL (m must be 0):  the neighbours of the n points among themselves, the pair (i, i) skipped
 *                             by index (a duplicate point with another index is a neighbour at 0);
 *                             rows = n, k <= n - 1
 *   Z != NULL:                the neighbours in X of the m points Z (m x d, column-major, ldz >= m), no
 *                             pair skipped; rows = m, k <= n
 * idx (int32) and d2 are rows x k host blocks, column-major, ldi, ldd >= rows: column c holds the
 * (c + 1)-th nearest and its squared distance.  The distance is always Euclidean — the kernel kind,
 * gamma, scale and nugget do not enter — in the Gram form of the operator, d2 = max((|x_i|^2 + |x_j|^2)
 * - 2 x_i.x_j, 0) on fp64 MFMA, so with Z == NULL d2(i, j) and d2(j, i) are the same bits.  Row i's
 * result is the k smallest under the total order (d2, j), the smaller index first on equal d2, written
 * ascending: it is unique, so it depends on neither the split count nor the CU count, two calls give
 * the same bits, and there are no atomics.  splits = 0: the column range is split by
 * rbl_kernel_cross_splits(rows, n, d); otherwise that many splits, 1 .. 64 and at most the stages of
 * the column range (64 points for d <= 16, 32 for d <= 64, else 16).  Runs on the context's stream (a
 * run in flight is waited for); extra device memory for the call only: the points of Z, the lists and
 * splits x rows x k entries of partial lists.
 * RBL_ERR_STATE without a kernel matrix; RBL_ERR_INVALID for k < 1, k > RBL_KNN_MAX, k beyond the
 * column points available, m < 1 with Z, m != 0 without, a NULL output, a leading dimension below its
 * block's rows, a non-finite entry of Z, or a bad splits — the context unchanged (a following rbl_apply
 * gives the bits of one before). */
#define RBL_KNN_MAX 64
int rbl_kernel_knn(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int k, int splits,
                   int32_t* idx, int64_t ldi, double* d2, int64_t ldd);
/* Milliseconds per neighbour search (the device part of rbl_kernel_knn alone, arguments as there):
 * one warm-up, then `reps` searches between two hipEvents. */
int rbl_bench_kernel_knn(rbl_ctx* ctx, int64_t m, const double* Z, int64_t ldz, int k, int splits,
                         int reps, double* ms);
/* Partial pivoted Cholesky of the kernel matrix held (csrc/pchol.hip): L L^T ~ A = diag(s) K diag(s), the
 * operator WITHOUT its nugget, from the points alone — a cheap CG preconditioner, landmark selection, a
 * Nystrom approximation.  With u = 2^-53 and R = max_rank:
 *   d_i = s_i^2 kappa(x_i, x_i) by the operator's diagonal rule (s_i^2 exactly for rbf and laplace),
 *   trace_0 = sum_i d_i, dmax0 = max_i d_i, floor = 4 (R + 2) u dmax0;
 *   step j = 0, 1, ...: the pivot p is the row with the largest d, the smaller index on a tie; stop with
 *   rank = j when j == R, or !(d_p > floor) (non-positive or NaN values, an indefinite poly kernel, exact
 *   duplicates), or trace_j <= tol trace_0; otherwise
 *     L[i, j] = (s_i s_p kappa(x_i, x_p) - sum_{l<j} L[i, l] L[p, l]) / sqrt(d_p)   (l ascending),
 *     L[p, j] = sqrt(d_p), L[i, j] = 0 exactly where d_i == 0 before the step (earlier pivots, rows whose
 *     residual was clamped away), d_i <- max(d_i - L[i, j]^2, 0), d_p <- 0, trace_{j+1} = sum_i d_i.
 * kappa is evaluated in the operator's Gram form in fp64 (one thread per row, ascending coordinates).
 * One launch per step, R + 1 enqueued back to back with one synchronisation at the end; every sum and
 * the pivot search run in an order that depends on n alone, without atomics or grid-wide
 * synchronisation: two calls give the same bits, on any device.  A step moves about 8 n (d4 + j + 3)
 * bytes, d4 = 4 ceil(d / 4).
 * L: host n x max_rank column-major, ldl >= n, columns at or beyond the rank zero; piv: max_rank int32,
 * -1 past the rank; trace: max_rank + 1 doubles (trace_0 .. trace_rank, the last repeated past the
 * rank); *rank_out the rank.  Any output may be NULL.  Runs on the context's stream (a run in flight is
 * waited for); device memory for the call only: L, d and the workgroups' partial records.
 * RBL_ERR_STATE without a kernel matrix; RBL_ERR_INVALID for max_rank outside [1, min(n,
 * RBL_PCHOL_MAX_RANK)], tol not finite or outside [0, 1), or ldl < n with L given — every rejection
 * before any allocation, the context unchanged (a following rbl_apply gives the bits of one before). */
#define RBL_PCHOL_MAX_RANK 256
int rbl_kernel_pchol(rbl_ctx* ctx, int max_rank, double tol, double* L, int64_t ldl, int32_t* piv,
                     double* trace, int* rank_out);
/* Milliseconds per factorisation at tol = 0 (the device part of rbl_kernel_pchol alone): one warm-up,
 * then `reps` factorisations between two hipEvents. */
int rbl_bench_kernel_pchol(rbl_ctx* ctx, int max_rank, int reps, double* ms);
/* Kernel-matrix derivative product over the points of the kernel matrix held:
 *     U (n x b) = (Phi o A B^T) Q,    Phi_ij = phi(x_i, x_j),    (A B^T)_ij = sum_k A_ik B_jk,
 * A and B n x r, Q n x b, host column-major blocks like rbl_kernel_cross (lda, ldb, ldq, ldu >= n).
 * With d2 the Gram-form squared distance of the operator (0 on the diagonal), t = gamma x_i^T x_j +
 * coef0 and q = degree, phi is
 *   RBL_KWEIGHT_VALUE   kappa
 *   RBL_KWEIGHT_DGAMMA  d kappa / d gamma:  rbf -d2 kappa, laplace -sqrt(d2) kappa, poly q x_i^T x_j t^(q-1)
 *   RBL_KWEIGHT_DSCALE  psi with d kappa / d log s_k = psi (x_ik - x_jk)^2 (rbf, laplace) or psi x_ik x_jk
 *                       (poly) at unit coordinate scales:  rbf -2 gamma kappa, laplace -gamma kappa /
 *                       sqrt(d2) and 0 where d2 == 0, poly 2 q gamma t^(q-1)
 * so sum_ij M_ij dK_ij / d theta for a low-rank M = A B^T is a few O(n d) host sums over one product
 * (theta = gamma: Q = 1; theta = log s_k: Q = [X, 1]).  Neither the scale nor the nugget of the operator
 * enters; fold a scale into A and B.  Phi o A B^T is never stored: a_i . b_j is one more Gram-form inner
 * product of the pair-tile scheme, all on fp64 MFMA, one launch per column chunk (32; a last chunk of 17 ..
 * 31 columns zero-padded to 32, of 1 .. 16 to 16), the column range not split.  Fixed summation order, no atomics: two calls
 * give the same bits, and with A = B = ones (r = 1), RBL_KWEIGHT_VALUE and b a multiple of 16 the
 * result has the bits of rbl_apply on the operator without scale and nugget.
 * RBL_ERR_STATE without a kernel matrix; RBL_ERR_INVALID for an unknown mode, r < 1 or
 * 4 ceil(d / 4) + 4 ceil(r / 4) > RBL_KERNOP_MAX_DIM, b outside [1, RBL_MAX_BLOCK], a NULL pointer, a
 * leading dimension below n, or a non-finite entry of A, B or Q — the context unchanged (a following
 * rbl_apply gives the bits of one before). */
#define RBL_KWEIGHT_VALUE   0
#define RBL_KWEIGHT_DGAMMA  1
#define RBL_KWEIGHT_DSCALE  2
int rbl_kernel_hadamard(rbl_ctx* ctx, int mode, int r, const double* A, int64_t lda, const double* B,
                        int64_t ldb, int b, const double* Q, int64_t ldq, double* U, int64_t ldu);
/* Milliseconds per derivative product of the matrix held with device-resident N(0,1) factors of r
 * columns and a block of b columns (the device part of rbl_kernel_hadamard alone): one warm-up, then
 * `reps` products between two hipEvents. */
int rbl_bench_kernel_hadamard(rbl_ctx* ctx, int mode, int r, int b, int reps, double* ms);
/* k-means on the device (csrc/kmeans.hip): Lloyd's iteration and k-means++ seeding over n points in d
 * dimensions, fp64, one GPU.  The points are the context's own, beside whatever matrix it holds:
 * setting or clearing them leaves the matrix, the basis and every option as they were.
 *
 * rbl_kmeans_set_points: X n x d column-major with leading dimension ldx >= n (host), 1 <= n < 2^31 - 64,
 * 1 <= d <= RBL_KERNOP_MAX_DIM, every entry finite; copied to the device (row-major, the columns
 * zero-padded to a multiple of 4, with their squared norms).  Replaces points set before.
 * rbl_kmeans_clear: releases them (no error when none are set).
 *
 * Distances are taken in the Gram form of rbl_kernel_knn,
 *     d2(i, j) = max((|x_i|^2 + |c_j|^2) - 2 x_i.c_j, 0),
 * the inner product a fixed-order fp64 MFMA chain, and a point goes to the centre with the smallest
 * (d2, j): the smaller index wins a tie.  Centre X first where its mean is far from 0.  Sums, counts,
 * inertia and the number of changed labels are added in an order that depends on (n, d, c) alone,
 * without atomics: two calls give the same bits, on any device.
 *
 * rbl_kmeans_run: C0 c x d column-major (ldc0 >= c), 1 <= c <= RBL_KMEANS_MAX_CLUSTERS, c <= n.  At
 * iteration t = 0, 1, ...: assign to C_t (labels_t, counts_t, inertia_t = sum_i d2(i, label_i),
 * changed_t = #{i: label_i differs from iteration t - 1}); stop with *converged_out = 1 if t >= 1 and
 * changed_t = 0; with 2 if t >= 1, tol > 0 and |C_t - C_{t-1}|_F^2 <= tol; with 0 if t = max_iter;
 * otherwise C_{t+1}: centre_j = (sum of its points) / count_j by an IEEE division, a centre with
 * count_j = 0 keeping its value.  Returned: the consistent triple labels_t (n int32), C_t (c x d
 * column-major, ldc >= c) and inertia_t, with counts_t (c int64) and *n_iter_out = t.  max_iter = 0
 * assigns only.  Any output may be NULL.  The host reads three doubles per iteration; nothing of size n
 * crosses PCIe inside the loop.
 *
 * rbl_kmeans_seed: plain k-means++ from the c uniforms u_r in [0, 1): round 0 picks
 * min(floor(u_0 n), n - 1); round r keeps w_i = min over the picked points of d2(i, .), 0 by index for a
 * picked point, and picks the smallest i whose inclusive prefix sum of w (a fixed order, a function of
 * n alone) exceeds u_r total — the smallest index not yet picked when total = 0.  picked_out: c int32
 * indices into the points.
 *
 * RBL_ERR_STATE when no points are set; RBL_ERR_INVALID for d or c out of range, c > n, a NULL input,
 * a leading dimension below its rows, a non-finite point, centre, uniform or tol, a uniform outside
 * [0, 1), tol < 0 or max_iter < 0 — the context and the stored points unchanged. */
#define RBL_KMEANS_MAX_CLUSTERS 256
int rbl_kmeans_set_points(rbl_ctx* ctx, int64_t n, int d, const double* X, int64_t ldx);
int rbl_kmeans_clear(rbl_ctx* ctx);
int rbl_kmeans_seed(rbl_ctx* ctx, int c, const double* uniforms, int32_t* picked_out);
int rbl_kmeans_run(rbl_ctx* ctx, int c, const double* C0, int64_t ldc0, int max_iter, double tol,
                   int32_t* labels_out, double* centers_out, int64_t ldc, int64_t* counts_out,
                   double* inertia_out, int* n_iter_out, int* converged_out);
/* Milliseconds per Lloyd iteration (assignment, update, reduction and the new centres; the device part
 * of rbl_kmeans_run alone) over the points set, every iteration against the centres C0: one warm-up,
 * then `reps` iterations between two hipEvents. */
int rbl_bench_kmeans_iter(rbl_ctx* ctx, int c, const double* C0, int64_t ldc0, int reps, double* ms);
int rbl_gen_matrix_hashwindow(rbl_ctx* ctx, int64_t n, int64_t halfwidth, double density,
                              uint64_t seed, int nplant, const double* plant);
/* Device-side generator of the seeded symmetric R-MAT matrix (BASELINE
 * config 4): `edges` draws descend `scale` levels with quadrant probabilities (a, b, c,
 * 1-a-b-c); draws with an id >= n or a self loop are dropped, the rest enter as (r,c) and
 * (c,r), duplicates merged; off-diagonal values 2u-1 from the pair hash (as hash-window),
 * every diagonal entry present (hash value + planted spectrum, as hash-window).  Rows are
 * split over the ranks by nonzeros.  NumPy restatement: oracle/matgen.py rmat_csr. */
int rbl_gen_matrix_rmat(rbl_ctx* ctx, int64_t n, int scale, int64_t edges, double a, double b,
                        double c, uint64_t seed, int nplant, const double* plant);
/* Device-side generator of a circuit-like SPD matrix of SuiteSparse G3_circuit's shape
 * (BASELINE config 3; the real file is not shipped): a weighted graph Laplacian on a 5-point
 * stencil over rows of `width` nodes, each edge (lo,hi) kept iff hash(seed,lo,hi) < p_edge,
 * weight 0.5 + uniform[0,1) from the same hash; diagonal 0.01 + the kept weights (+ plant[l]
 * at node l*floor(n/nplant)); node i is scattered to row/column scatter(i), a seeded Feistel
 * bijection of [0,n), so the pattern has no band (the gather SpMM runs).  n = 1,585,478,
 * width 1259, p_edge 0.95873 give G3_circuit's 7.66 M nonzeros.  Rows split uniformly over
 * the ranks.  NumPy restatement: oracle/matgen.py circuit_like_csr. */
int rbl_gen_matrix_circuit(rbl_ctx* ctx, int64_t n, int64_t width, double p_edge, uint64_t seed,
                           int nplant, const double* plant);
int rbl_matrix_info(rbl_ctx* ctx, int64_t* n, int64_t* row_begin, int64_t* row_end,
                    int64_t* nnz_local);
/* Original (generator) id of each local row: r0 + i, or perm^-1(r0 + i) for a matrix generated
 * with RBL_OPT_RELABEL.  ids: n_local int64. */
int rbl_row_ids(rbl_ctx* ctx, int64_t* ids);
/* Download the local CSR (0-based) — test/inspection only. */
int rbl_get_matrix_csr(rbl_ctx* ctx, int64_t* rowptr, int32_t* colind, double* val);
/* Y = A X for a host n_local x b column-major block (the operator of RBL_gpu.jl:176,
 * `mul!(U, Ag, Qg_d)`), through the same SpMM kernels as rbl_step (multi-rank: with the
 * halo exchange); with an update set (rbl_set_lowrank) Y = (A + P S P^T) X.  Allocates its own
 * device buffers. */
int rbl_apply(rbl_ctx* ctx, int b, const double* X, double* Y);
/* Which SpMM kernel rbl_step / rbl_apply use for block size b under the current option:
 * 1 = global-gather CSR, 2 = LDS-window CSR (DPP), 3 = LDS-densified band on fp64 MFMA,
 * 4 = dense panel GEMM (rbl_set_matrix_dense), 5 = band-tile format on fp64 MFMA,
 * 6 = segmented gather (unstructured patterns, b in {16, 32}), 7 = column panels,
 * 8 = rectangular gather pair (rbl_set_matrix_normal, every b),
 * 9 = implicit kernel matrix (rbl_set_matrix_kernel, every b). */
int rbl_spmm_kernel_for(rbl_ctx* ctx, int b);
/* The device format the matrix is held in: 0 = CSR only, 1 = band tiles (16 x (16 + 2H)
 * doubles), 2 = packed band tiles (RBL_BT_PACK=1), 3 = half band tiles (A symmetric bit for
 * bit: diagonal block + right strip, the left part transposed back in the kernel, same
 * results as 1; opt-in with RBL_BT_HALF=1), 4 = dense panels, 5 = rectangular B as two CSRs
 * (B and B^T, rbl_set_matrix_normal), 6 = the points of an implicit kernel matrix
 * (rbl_set_matrix_kernel). */
int rbl_matrix_format(rbl_ctx* ctx);

/* ---- Krylov run -----------------------------------------------------------------------
 * rbl_start replaces RBL_gpu.jl:213-214 (`Qg_d = CUDA.randn(n,b); Qg_d = qr(Ag*Qg_d).Q`)
 * and the buffer planning of RBL_gpu.jl:95-104 (the whole basis lives in HBM).
 * `omega` is the local n_local x b column-major start block, or NULL for a device
 * counter-based N(0,1) draw from `seed`.  basis_bits: 64 (fp64 basis) or 32 (the mixed
 * mode of RBL_gpu.jl with FLOAT = Float32, any b: Krylov blocks and their partial /
 * local reorthogonalisation in fp32 on fp32 MFMA; A Q, the 3-term update, QR, A_i, B_i and
 * the Ritz projection in fp64 from the widened blocks). */
int rbl_start(rbl_ctx* ctx, int b, int max_blocks, int basis_bits, const double* omega,
              uint64_t seed);
/* One block Lanczos step i (1-based) — RBL_gpu.jl:149-161 for i == 1 and :163-184 for
 * i >= 2: partial reorth of Q_i, Q_{i-1} against Q_1..Q_{i-2} when bit 0 of `part_reorth`
 * is set (the reference sets it for even i; restarted.jl for i % 3 == 0), preceded by
 * their reorth against the locked vectors when bit 1 is set (restarted.jl:54-55; at i == 1
 * Q_1 alone, :41; fp64 basis only), local reorth, U = A Q_i - Q_{i-1} B_i^T,
 * A_i = Q_i^T U, U -= Q_i A_i, Q_{i+1} B_{i+1} = qr(U).  A_out/B_out: b x b column-major
 * host buffers receiving A_i and B_{i+1} (upper triangular) — the only per-step traffic. */
int rbl_step(rbl_ctx* ctx, int i, int part_reorth, double* A_out, double* B_out);
/* rbl_step without the per-step host round trip: the step is only enqueued; A_i, B_{i+1}
 * and its status are stashed in pinned memory and handed over by rbl_fetch.  Steps may be
 * enqueued back to back (the GPU never idles between them); the host fetches where it needs
 * the T band (the reference pushes every step, RBL_gpu.jl:185/193, but reads it only at the
 * convergence checks, :186-189).  A QR breakdown surfaces at the fetch. */
int rbl_step_async(rbl_ctx* ctx, int i, int part_reorth);
/* Wait for steps up to i1 - 1 and return those of [i0, i1) (i0 = the first unfetched step);
 * steps enqueued after i1 - 1 keep running (the host may enqueue ahead of a convergence check
 * and work on the T band meanwhile: with partial reorth at even steps, the steps after an even
 * i1 - 1 never touch blocks 1..i1-1):
 * A_out / B_out receive (i1-i0) consecutive b x b column-major blocks, status_out (may be
 * NULL) each step's status (RBL_OK, RBL_WARN_QR_SHIFTED, RBL_ERR_NUMERIC).  Returns
 * RBL_ERR_NUMERIC if any of them broke down, else RBL_OK.  rbl_step refuses to run while
 * asynchronous steps are unfetched. */
int rbl_fetch(rbl_ctx* ctx, int i0, int i1, double* A_out, double* B_out, int* status_out);
/* Ritz vectors — RBL_gpu.jl:106-132 / RBL.jl:61-71 in fp64:  V = [Q_1..Q_nblocks] S.
 * S: (nblocks*b) x k column-major (host); V_out: n_local x k column-major (host). */
int rbl_ritz(rbl_ctx* ctx, int nblocks, int k, const double* S, double* V_out);
/* Copy basis block j (1-based) to the host (n_local x b column-major) — tests only. */
int rbl_get_block(rbl_ctx* ctx, int j, double* Q_out);
int rbl_num_blocks(rbl_ctx* ctx);

/* ---- Chebyshev-filtered runs: the smallest or largest eigenpairs ---------------------------
 * (No reference equivalent: the reference returns the largest-magnitude pairs only.)
 * rbl_set_filter: with degree >= 1 every later rbl_start, rbl_step, rbl_step_async and restart
 * cycle runs block Lanczos on
 *     p(A) = T_d((A - c I) / e) / T_d((ref - c) / e),   c = (lo + hi) / 2,  e = (hi - lo) / 2,
 * |p| <= 1 / |T_d((ref - c)/e)| on the damped interval [lo, hi], p(ref) = 1 and growing outside:
 * the eigenvalues of A beyond `ref`'s end of the spectrum become the largest-magnitude ones of
 * p(A).  Applied by the scaled three-term recurrence of Zhou and Saad (nothing overflows):
 *     s_1 = e / (ref - c),  Y_1 = (s_1 / e) (A X - c X),
 *     s' = 1 / (2 / s_1 - s),  Y_j = (2 s' / e) (A Y_{j-1} - c Y_{j-1}) - s s' Y_{j-2},  s = s',
 * each term one SpMM (whichever kernel the matrix runs) and one row pass.  The step then forms
 * U = p(A) Q_i - Q_{i-1} B_i^T; T holds p's eigenvalues, the Ritz vectors are A's eigenvectors
 * (rbl_ritz_project / rbl_ritz_finish recover A's eigenvalues).  degree 0 clears the filter:
 * every path is then the unfiltered one, bit for bit.  rbl_apply stays the plain A X.
 * Limits (RBL_ERR_INVALID, before any collective or allocation): one rank only; the fp64 basis
 * only (rbl_start with basis_bits = 32 while a filter is set); no rectangular B; degree >= 0;
 * lo < hi; ref outside [lo, hi]; finite arguments. */
int rbl_set_filter(rbl_ctx* ctx, int degree, double lo, double hi, double ref);
/* rbl_set_filter_series: the Krylov operator becomes a general Chebyshev series
 *     p(A) = sum_{j=0..degree} mu[j] T_j((A - c I) / e),   c = (lo + hi) / 2,  e = (hi - lo) / 2,
 * with [lo, hi] enclosing the WHOLE spectrum of A (T_j grows exponentially outside it) — an
 * operator that can peak inside the spectrum (rbl.interior: the eigenpairs nearest a target).
 * Applied by T_0 = X, T_1 = (A X - c X) / e, T_j = (2 / e)(A T_{j-1} - c T_{j-1}) - T_{j-2}: each
 * term one SpMM and one fused row pass that forms T_j and adds mu[j] T_j to the result, through
 * three work blocks.  mu has degree + 1 entries and is copied.  Setting either kind of filter
 * replaces the other; rbl_set_filter(ctx, 0, ...) clears both.  rbl_apply_filter, rbl_start,
 * rbl_step and rbl_step_async apply whichever is set; rbl_apply stays the plain A X.
 * Limits (RBL_ERR_INVALID, the context stays usable): 1 <= degree <= 65535; lo < hi, both finite;
 * mu non-NULL, every entry finite; one rank only; the fp64 basis only (also rbl_start with
 * basis_bits = 32 while the series is set); no rectangular B. */
int rbl_set_filter_series(rbl_ctx* ctx, int degree, double lo, double hi, const double* mu);
/* Y = p(A) X for a host n_local x b column-major block (the convention of rbl_apply), with the
 * filter set; RBL_ERR_STATE without one.  Timed under "AQ". */
int rbl_apply_filter(rbl_ctx* ctx, int b, const double* X, double* Y);
/* Diagnostics: the time per pass (ms, hipEvents, mean over `reps` after one warm-up) of the fused
 * row pass of a series term and of the two plain row passes it replaces (the term, then the
 * accumulation), each over blocks of `len` doubles allocated for the call. */
int rbl_bench_series_pass(rbl_ctx* ctx, int64_t len, int reps, double* fused_ms, double* pair_ms);
/* rbl_cheb_moments: the Chebyshev moments of A over a block of b vectors (the kernel polynomial
 * method: spectral density, eigenvalue counts; rbl.density),
 *     mom_out[j + (2 degree + 1) c] = x_c^T T_j((A - cI) / e) x_c,   j = 0..2 degree,
 * c = (lo + hi) / 2, e = (hi - lo) / 2, with [lo, hi] enclosing the WHOLE spectrum of A (|m_j| <=
 * m_0 then; T_j grows exponentially outside it).  X: host n_local x b column-major, or NULL for
 * the counter-based N(0,1) draw of rbl_start (the same seed gives the same block).  mom_out: host,
 * (2 degree + 1) x b column-major.  degree SpMMs give 2 degree + 1 moments: with t_j = T_j x from
 * the recurrence of rbl_set_filter_series,
 *     m_0 = <x,x>,  m_1 = <t_1,x>,  m_2j = 2 <t_j,t_j> - m_0,  m_(2j-1) = 2 <t_j,t_(j-1)> - m_1,
 * each term one SpMM and one row pass that forms t_j and the per-column partials of both dots
 * (a fixed summation order, no atomics: two calls give the same bits).  The dots of all terms stay
 * on the device until one copy at the end.  The call allocates its own three work blocks: the
 * Krylov basis, a run in progress and a filter that is set are untouched.  Timed under "AQ".
 * Limits (RBL_ERR_INVALID, before any allocation; the context stays usable): 1 <= b <=
 * RBL_MAX_BLOCK; 1 <= degree <= 65535; lo < hi, both finite; mom_out non-NULL; one rank only; no
 * rectangular B.  RBL_ERR_STATE without a matrix. */
int rbl_cheb_moments(rbl_ctx* ctx, int b, int degree, double lo, double hi, const double* X,
                     uint64_t seed, double* mom_out);
/* Diagnostics: the time per pass (ms, hipEvents, mean over `reps` after one warm-up) of the moment
 * row pass of a middle term with its partial-sum reduction, over blocks of len_rows x b doubles
 * allocated for the call. */
int rbl_bench_moment_pass(rbl_ctx* ctx, int64_t len_rows, int b, int reps, double* ms);
/* rbl_cheb_diag: the diagonals of nf matrix functions at once (subgraph centrality diag exp(A),
 * heat-kernel signatures diag exp(-t L) at many t, the local density of states at many energies;
 * rbl.funm), by the probing estimator over a block of b vectors x_c:
 *     num_out[row + n_local e] = sum_c x_c[row] (p_e(A) x_c)[row],   den_out[row] = sum_c x_c[row]^2,
 *     p_e(A) = sum_{j=0..degree} coef[j + (degree + 1) e] T_j((A - cI) / e'),  e < nf,
 * c = (lo + hi) / 2, e' = (hi - lo) / 2, with [lo, hi] enclosing the WHOLE spectrum of A; num / den
 * estimates diag p_e(A) (exactly, when the x_c are identity columns).  coef: host, (degree + 1) x nf
 * column-major (function e's coefficients contiguous); it is copied.  X: host n_local x b
 * column-major, or NULL for a block drawn on the device from `seed`: probe = RBL_PROBE_GAUSS the
 * counter-based N(0,1) draw of rbl_start, RBL_PROBE_SIGN its signs (+-1, 0 -> +1: Rademacher, den =
 * b exactly).  probe is checked but not used when X is given.  num_out: host, n_local x nf
 * column-major, rows in the order rbl_apply returns them; den_out: host, n_local.
 * ONE recurrence serves all nf functions: `degree` SpMMs (the operator routine of every other entry
 * point, so a low-rank update that is set applies) and after each ONE row pass that forms t_j,
 * s[row] = sum_c X[row][c] t_j[row][c] and D[row][e] += coef[j][e] s[row] — 40 + 16 nf / b bytes per
 * element and term, against 48 for every function through rbl_apply_filter.  The row sums run in a
 * fixed order with no atomics (each thread its slot's columns, the row's slots ascending through
 * LDS, one owner thread per element of D): two calls give the same bits.  The call allocates its
 * own four work blocks (X is kept beside the three of the recurrence), D and the device copy of
 * coef: the Krylov basis, a run in progress and a filter or series that is set are untouched.
 * Timed under "AQ".
 * b <= 256: a row of the block is then at most 256 slots of the row pass, which finishes it inside
 * one tile pass of a workgroup; no cross-chunk row accumulation exists.
 * Limits (RBL_ERR_INVALID, before any allocation; the context stays usable): 1 <= b <= 256;
 * 1 <= degree <= 65535; 1 <= nf <= 32; lo < hi, both finite; coef non-NULL, every entry finite;
 * probe RBL_PROBE_GAUSS or RBL_PROBE_SIGN; num_out and den_out non-NULL; one rank only; no
 * rectangular B.  RBL_ERR_STATE without a matrix. */
#define RBL_PROBE_GAUSS 0   /* the N(0,1) draw of rbl_start */
#define RBL_PROBE_SIGN  1   /* its signs: Rademacher */
int rbl_cheb_diag(rbl_ctx* ctx, int b, int degree, double lo, double hi, int nf, const double* coef,
                  const double* X, uint64_t seed, int probe, double* num_out, double* den_out);
/* Diagnostics: the time per pass (ms, hipEvents, mean over `reps` after one warm-up) of the
 * diagonal row pass of a middle term, over blocks of len_rows x b doubles and a len_rows x nf D
 * allocated for the call.  1 <= b <= 256, 1 <= nf <= 32. */
int rbl_bench_diag_pass(rbl_ctx* ctx, int64_t len_rows, int b, int nf, int reps, double* ms);

/* ---- implicit symmetric low-rank update: the operator A + P S P^T ----------------------------
 * (No reference equivalent.)  rbl_set_lowrank: with P (n x r, host, column-major) and S (r x r,
 * host, column-major, symmetric) every later n-sized product of the library runs on
 *     Op = A + P S P^T
 * — the modularity matrix A - d d^T / (2m) (r = 1), Hotelling deflation A - V Theta V^T past the
 * eigenpairs already found, a double-centred kernel matrix H K H (r = 2, S not diagonal) — which
 * is dense and never formed.  All of them go through one operator routine, so rbl_apply,
 * rbl_start, rbl_step, rbl_step_async, the restarted entry points, both Chebyshev filters
 * (rbl_apply_filter: p(Op)), rbl_cheb_moments, rbl_cheb_diag and rbl_ritz_project / rbl_ritz_finish (W = Op V,
 * residuals ||Op v - theta v||) all see Op.  After the SpMM and its fused 3-term epilogue three
 * passes run in stream order, with no host round trip:
 *     w = P^T X (r x b),   c = S w,   U[row, :] += P[row, :] c   (rows < n_local)
 * every sum in a fixed order (no atomics): two calls give the same bits.  P and S are copied (P
 * to n x rp doubles on the device, rp = r rounded up to one of 2, 4, 6, 8, 12, 16, 24, 32); the
 * caller's arrays are not kept.  Set it before rbl_start: a run in flight is waited for, and its
 * basis belongs to the operator it was built with.  A block step forms A_i = Q_i^T U from the
 * final U with its own Gram (the band-tile kernel's fused A_i partials predate the update).
 * r = 0 or P = NULL clears the update: results are then bit for bit those of a context that never
 * had one, with no extra launch.  Setting any matrix clears it too.
 * Limits, each checked before any allocation, the context and an earlier update staying as they
 * were: RBL_ERR_STATE without a matrix, with a rectangular B (rbl_set_matrix_normal) or while the
 * current run has the fp32 basis; RBL_ERR_INVALID on a context with several ranks, for r outside
 * [1, 32], S = NULL, a non-finite entry of P or S, or S != S^T (compared exactly); rbl_start with
 * basis_bits = 32 while an update is set returns RBL_ERR_INVALID.  Dense and sparse A, any
 * b <= RBL_MAX_BLOCK.  Extra device memory: n x rp x 8 B and under 8 workgroups per CU x rp x b x 8 B. */
int rbl_set_lowrank(rbl_ctx* ctx, int r, const double* P, const double* S);
/* The update set: *r_out its rank, P_out (n x r) and S_out (r x r) column-major, exactly the
 * values passed (any of the three may be NULL; call once for r, then with buffers).
 * RBL_ERR_STATE when no update is set. */
int rbl_get_lowrank(rbl_ctx* ctx, int* r_out, double* P_out, double* S_out);
/* Diagnostics: the time per pass (ms, hipEvents, mean over `reps` after one warm-up) of the
 * projection w = P^T X (its partial-sum reduction included) and of the update U += P c, over
 * scratch blocks of rows x b doubles and a rows x r factor allocated for the call. */
int rbl_bench_lowrank_pass(rbl_ctx* ctx, int64_t rows, int b, int r, int reps, double* project_ms,
                           double* update_ms);

/* Preconditioned conjugate gradients: (Op + shift I) X = B for a symmetric positive definite
 * Op + shift I, Op whatever rbl_apply applies (sparse, dense or kernel matrix, with the update of
 * rbl_set_lowrank when one is set).  The b columns run their own Hestenes-Stiefel recurrence and
 * share one product per iteration; every per-column scalar stays on the device, a column is frozen
 * on the device once |r| <= tol |b| (its x is not stored again), and the host only reads the count
 * of active columns every check_every iterations — the returned bits do not depend on check_every.
 * All sums run in a fixed order, no atomics: two calls give the same bits.
 *
 * rbl_set_precond_lowrank: the preconditioner M^-1 = I + V diag(dv) V^T, V n x r column-major with
 *   orthonormal columns (not checked), 1 <= r <= 32, dv[i] > -1 finite; both copied to the device,
 *   in buffers of their own (an rbl_set_lowrank update may be set at the same time).  Replaces an
 *   earlier one; rbl_clear_precond, setting any matrix and rbl_free drop it.  RBL_ERR_INVALID
 *   (several ranks, a rectangular B, r outside [1, 32], a NULL or non-finite argument) and
 *   RBL_ERR_STATE (no matrix) leave the context as it was.
 * rbl_solve: B and X n x b column-major on the host, 1 <= b <= RBL_MAX_BLOCK.  use_x0 != 0: X holds
 *   the starting guess (one extra product forms r = b - (Op + shift) x0); else x0 = 0.  Stops when
 *   every column is frozen or after max_iter iterations (1 .. 65535; with coef at most 4096).  Per
 *   column: iters, status (RBL_SOLVE_CONVERGED; RBL_SOLVE_MAX_ITER; RBL_SOLVE_NOT_POSDEF: p^T (Op +
 *   shift) p <= 0 or not finite — the column keeps the x it had, and the call still returns RBL_OK),
 *   resid = |b - (Op + shift I) x| / |b| of the returned x, from one final product (|b| = 0: the
 *   absolute norm; a zero column returns x = 0, converged, 0 iterations).  coef (NULL or 2 max_iter b
 *   doubles): column c's alpha_j at coef[c * 2 max_iter + 2 j] and beta_j one further, j < iters[c],
 *   zero beyond — the Lanczos tridiagonal of (Op + shift I, b_c) (rbl.cg_tridiag).
 *   Timed under "AQ" (the products) and "3-term" (the row passes); while RBL_OPT_TIMERS is on the
 *   host looks at the active count at least every 64 iterations, so the timing events in flight stay
 *   bounded whatever check_every is.
 *   Limits (before any allocation; the context stays usable): RBL_ERR_INVALID for b, max_iter or
 *   check_every (>= 1) out of range, tol outside (0, 1), a non-finite shift, a NULL pointer, several
 *   ranks or a rectangular B; RBL_ERR_STATE without a matrix or while the run has the fp32 basis.
 *   Device memory: 5 blocks of n x b doubles for the call. */
#define RBL_SOLVE_CONVERGED  0
#define RBL_SOLVE_MAX_ITER   1
#define RBL_SOLVE_NOT_POSDEF 2
int rbl_set_precond_lowrank(rbl_ctx* ctx, int r, const double* V, const double* dv);
int rbl_clear_precond(rbl_ctx* ctx);
int rbl_solve(rbl_ctx* ctx, int b, const double* B, double* X, double shift, double tol, int max_iter,
              int check_every, int use_x0, int* iters, int* status, double* resid, double* coef);
/* Diagnostics: ms[0..2] = the time per pass (hipEvents, mean over `reps` after one warm-up) of the
 * dot pass, the update pass (each with its partial-sum reduction) and the direction pass of one CG
 * iteration on scratch blocks of len_rows x b doubles; r > 0: with a preconditioner of rank r, the
 * direction pass then includes the projection V^T r. */
int rbl_bench_cg_pass(rbl_ctx* ctx, int64_t len_rows, int b, int r, int reps, double* ms);

/* Rayleigh-Ritz on A with true residuals (also without a filter).
 * rbl_ritz_project: V = [Q_1..Q_nblocks] S (S: (nblocks*b) x k column-major, host; orthonormal
 *   columns) and W = A V (the plain operator, never the filter; with rbl_set_lowrank A + P S P^T)
 *   are formed and kept on the device; H_out (k x k
 *   column-major, host) = V^T W.  k <= RBL_MAX_BLOCK; one rank; replaces an earlier projection.
 * rbl_ritz_finish: with the host's eigendecomposition H = Y diag(theta) Y^T (Y: k x k
 *   column-major), V_out (n_local x k column-major) = V Y and resid_out[j] =
 *   || W y_j - theta_j V y_j ||_2, the true residual of the pair (theta_j, V y_j) — per-workgroup
 *   partial sums added in a fixed order, no atomics.  Frees V and W.  RBL_ERR_STATE without a
 *   preceding rbl_ritz_project (of the same k). */
int rbl_ritz_project(rbl_ctx* ctx, int nblocks, int k, const double* S, double* H_out);
int rbl_ritz_finish(rbl_ctx* ctx, int k, const double* Y, const double* theta, double* V_out,
                    double* resid_out);
/* rbl_ritz_finish for a subset of the pairs: after rbl_ritz_project of width kproj, Y holds k <=
 * kproj chosen eigenvector columns of H (kproj x k column-major) and theta their k eigenvalues;
 * V_out is n_local x k and resid_out has k entries.  kproj == k is rbl_ritz_finish. */
int rbl_ritz_finish_cols(rbl_ctx* ctx, int kproj, int k, const double* Y, const double* theta,
                         double* V_out, double* resid_out);

/* ---- restarted variants (restarted.jl: RBL_gpu_restarted / RBL_restarted) ---------------
 * Locked Ritz vectors live on the device (Qlock_gpu); fp64 basis runs only.
 * rbl_restart: the next cycle starts from Q_1 = [Q_1..Q_nblocks] S (S: (nblocks*b) x b
 *   column-major), no QR — restarted.jl:131-132 `Qi = recover_eigvec(...)`; the locked set
 *   is kept, the block count resets to 1.
 * rbl_lock: append the nvec Ritz vectors [Q_1..Q_nblocks] S (S: (nblocks*b) x nvec) to the
 *   locked set — restarted.jl:121-126.  rbl_start empties the locked set.
 * rbl_reorth_last: the end-of-cycle reorth of Q_nblocks, Q_{nblocks-1} (flags as rbl_step's
 *   part_reorth) — restarted.jl:100-102. */
int rbl_restart(rbl_ctx* ctx, int nblocks, const double* S);
int rbl_lock(rbl_ctx* ctx, int nblocks, int nvec, const double* S);
int rbl_num_locked(rbl_ctx* ctx);
int rbl_get_locked(rbl_ctx* ctx, double* V_out);  /* n_local x num_locked column-major */
int rbl_reorth_last(rbl_ctx* ctx, int nblocks, int flags);

/* ---- thick restart: block Lanczos in a bounded basis ------------------------------------------
 * (No reference equivalent: restarted.jl restarts from one Ritz vector with explicit locking.)
 * After m = nblocks steps the run holds A Q = Q T + Q_{m+1} B_{m+1} E_m^T, Q = [Q_1 .. Q_m].  With
 * the host's T = S Theta S^T, p = keep_blocks * b chosen columns S_p and W = B_{m+1} S_p[last b
 * rows, :] the Ritz block Y = Q S_p satisfies  A Y = Y Theta_p + Q_{m+1} W  — a Krylov relation
 * again, over the basis [Y_1 .. Y_kb, Q_{m+1}] with the projected matrix diag(Theta_p) bordered by
 * W.  rbl_thick_restart turns the basis into that one, in stream order:
 *   slots 0 .. kb-1 <- [Q_1 .. Q_m] S (S: host, column-major, (m b) x (kb b)), IN PLACE: a workgroup
 *     owns whole rows and finishes every load of them before its first store, the accumulators of
 *     all kb b output columns staying in registers (b in {16, 32}: fp64 MFMA, each basis element
 *     read from HBM once; any other b: one thread per output column) — nothing of size n is
 *     allocated, which is the point of a memory-bounded run; a fixed summation order, no atomics:
 *     two calls give the same bits;
 *   slot kb <- the old slot m (Q_{m+1}), a device copy, bit for bit;
 *   W (host, column-major, b x (kb b)) is kept on the device for the next step;
 *   rbl_num_blocks becomes kb + 1, the cached local-reorth Gram is dropped, every step counts as
 *   fetched: the next legal call is rbl_step / rbl_step_async with i = kb + 1.
 * That step is the only one with a long recurrence (the "arrow" step):
 *     U = Op Q_{m+1} - [Y_1 .. Y_kb] W^T,  A_i = Q_{m+1}^T U,  U -= Q_{m+1} A_i,  Q_next B_next = qr(U)
 * with Op whatever operator is set (sparse on any SpMM kernel, dense, B^T B with or without a
 * shift, a low-rank update, a Chebyshev filter); the operator runs without its 3-term epilogue,
 * the subtraction is one tall-skinny GEMM over the kept run, A_i comes from the Gram of the final U
 * and the local reorth runs as its own pass.  Every later step is the ordinary 3-term step.
 * rbl_start, setting a matrix and rbl_restart clear a pending arrow step.  The locked set of the
 * restarted.jl path is untouched.
 * RBL_COMPRESS_MAX_COLS bounds kb b: a 64-row tile of 512 output columns is 128 fp64 accumulators
 * per lane over 4 waves, half of the 512 registers a lane has at one wave per SIMD (the rest hold
 * operands, the prefetched panel and addresses).
 * Refused before any change (the context stays usable, the basis is unchanged): RBL_ERR_INVALID
 * for S or W NULL, a non-finite entry of either, keep_blocks outside [1, nblocks), keep_blocks * b >
 * RBL_COMPRESS_MAX_COLS, or several ranks; RBL_ERR_STATE without an fp64 run, with the fp32 basis,
 * with a spilled basis (RBL_OPT_DEVICE_BLOCKS), with unfetched asynchronous steps, or when
 * nblocks + 1 != rbl_num_blocks. */
#define RBL_COMPRESS_MAX_COLS 512
int rbl_thick_restart(rbl_ctx* ctx, int nblocks, int keep_blocks, const double* S, const double* W);
/* Diagnostics: the time per pass (ms, hipEvents, mean over `reps` after one warm-up) of the
 * in-place compression of m synthetic rows x b blocks to keep_blocks blocks, and of the route
 * without it: ceil(keep_blocks b / 64) out-of-place tall-skinny GEMMs, each re-reading all m
 * blocks, into a rows x 64 scratch block.  Everything is allocated and zeroed for the call. */
int rbl_bench_compress_pass(rbl_ctx* ctx, int64_t rows, int b, int m, int keep_blocks, int reps,
                            double* inplace_ms, double* sliced_ms);

/* ---- timers --------------------------------------------------------------------------- */
int rbl_num_stages(void);
const char* rbl_stage_name(int stage);
int rbl_timers(rbl_ctx* ctx, double* ms, int nstages);
int rbl_reset_timers(rbl_ctx* ctx);
/* Stage times accumulate (ms, hipEvents on the context stream) while RBL_OPT_TIMERS is
 * set; names are the reference's TimerOutputs labels (RBL_gpu.jl:153-186: "AQ", "3-term",
 * "qr", "part reorth", "loc reorth", "Ritz vectors") plus "comm" (halo + all-reduce) and
 * "spill wait" (host spill: the stall on a block's copy-out).
 * rbl_synchronize waits for the context's stream and folds finished events into them. */
int rbl_synchronize(rbl_ctx* ctx);

/* Collectives this rank issued since the last reset (no reference equivalent: the reference is
 * single-GPU).  out[RBL_COMM_*] for the first nstats counters; reset != 0 zeroes them after the
 * read.  All-reduces are the b x b / (m b) x 2b Gram sums; exchanges the grouped halo
 * send/recv of Q rows before each SpMM (one rank: all zero). */
#define RBL_COMM_ALLREDUCE_CALLS 0
#define RBL_COMM_ALLREDUCE_BYTES 1
#define RBL_COMM_EXCHANGE_CALLS  2
#define RBL_COMM_SEND_BYTES      3
#define RBL_COMM_RECV_BYTES      4
#define RBL_COMM_NSTATS          5
/* the halo plan of the matrix held (set by rbl_set_matrix_* / the generators; reset keeps them):
 * RBL_COMM_HALO_PUSH 1 when the push/pull split runs (RBL_OPT_HALO_PUSH), and the Q rows per
 * SpMM summed over ranks that its setup predicted with the split (pulled + pushed) and with
 * the pull-all halo (0 on one rank or a banded A; the split's count also 0 when
 * RBL_OPT_HALO_PUSH is 0, which skips its evaluation) */
#define RBL_COMM_HALO_PUSH       5
#define RBL_COMM_PUSH_ROWS       6
#define RBL_COMM_PULL_ROWS       7
/* time in the collectives since the last reset, ns: host wall time inside the transport's calls
 * (all-reduces / halo exchanges; RCCL only enqueues, the shm and in-process stand-ins block),
 * and the hipEvent span each call holds its stream — the wait for the slowest peer included —
 * summed (recorded only while RBL_OPT_TIMERS is 1) */
#define RBL_COMM_ALLREDUCE_HOST_NS 8
#define RBL_COMM_EXCHANGE_HOST_NS  9
#define RBL_COMM_ALLREDUCE_DEV_NS  10
#define RBL_COMM_EXCHANGE_DEV_NS   11
int rbl_comm_stats(rbl_ctx* ctx, int64_t* out, int nstats, int reset);

/* All-gather of n int64 per rank from host memory: all[p*n + i] = rank p's mine[i] (one rank: a
 * copy).  A collective, ordered after the work already enqueued on the context (the host waits
 * for it).  The host loop uses it to take one decision for every rank — the convergence test
 * and the speculation depth of the next check (rbl.lanczos) — so that ranks whose host
 * eigensolves differ in the last bit still enqueue the same steps and collectives. */
int rbl_allgather_host(rbl_ctx* ctx, const int64_t* mine, int64_t* all, int n);

/* Which code path the block steps took, counted as the work is issued (since the last reset;
 * nstats entries, missing ones 0).  Stage timers cannot show this when ranks share a GPU (a
 * stage's events also span the other ranks' kernels); these counts are exact. */
#define RBL_PATH_SPMM            0  /* SpMM launches on a sparse A                              */
#define RBL_PATH_SPMM_LOC_FUSED  1  /* ... of which applied the local-reorth update to Q_i      */
#define RBL_PATH_LOC_SEPARATE    2  /* local-reorth updates run as their own pass              */
#define RBL_PATH_LOC_GRAM        3  /* local-reorth Grams not formed by the producing pass     */
#define RBL_PATH_LOCFIX_EDGES    4  /* rank-edge rows corrected before the halo exchange       */
#define RBL_PATH_LOCFIX_REST     5  /* range-edge rows corrected after a fused SpMM            */
#define RBL_PATH_SPMM_TWO_WAVE   6  /* SpMM launches served by the two-waves-per-SIMD kernel
                                       (variants build only; 0 in the product library)        */
#define RBL_PATH_RITZ_PIECES     7  /* rbl_ritz calls that formed V in row pieces on the side
                                       stream with the staged D2H behind them                  */
#define RBL_PATH_CLOC_3TERM      8  /* local-reorth coefficients taken from the 3-term pass
                                       (RBL_OPT_CLOC_DERIVE: M R1^-1 R2^-1)                    */
#define RBL_PATH_CLOC_REORTH     9  /* local-reorth coefficients derived through the partial
                                       reorth (RBL_OPT_CLOC_DERIVE: G - Cm^T Ci)               */
#define RBL_PATH_UPD32_TAKEN     10 /* partial-reorth updates the device gate sent to the fp32
                                       kernel (RBL_OPT_UPD32) ...                              */
#define RBL_PATH_UPD32_REFUSED   11 /* ... and those it kept on the fp64 kernel; both counted on
                                       the device and read back behind the context's stream    */
#define RBL_PATH_UPD32_SHADOW_READ  12 /* basis panels the fp32 update read from the fp32
                                          shadow (RBL_OPT_UPD32_SHADOW) ...                    */
#define RBL_PATH_UPD32_SHADOW_CONV  13 /* ... and panels it rounded and stored to it; both counted
                                          on the device like the two above                     */
#define RBL_PATH_UPD32_SHADOW_BYTES 14 /* bytes of the shadow the current run plan holds (0: none;
                                          a state, not a counter: a reset leaves it)           */
#define RBL_PATH_NSTATS          15
int rbl_path_stats(rbl_ctx* ctx, int64_t* out, int nstats, int reset);
/* Diagnostics: the value g of the RBL_OPT_UPD32 gate at block step i in out[i % 64] (n <= 64
 * entries; 0 where the gate has not run).  Waits for the context's stream. */
int rbl_upd32_gate_values(rbl_ctx* ctx, double* out, int n);
/* Diagnostics of RBL_OPT_UPD32_SHADOW: the number of leading blocks whose shadow slot holds
 * (float) of the block as it stands (0 without a shadow), and the shadow of block j (1-based as
 * rbl_get_block, j <= rbl_shadow_valid) as n_local x 32 floats ROW-major, whatever the layout on
 * the device.  Both wait for the context's stream. */
int rbl_shadow_valid(rbl_ctx* ctx);
int rbl_get_shadow_block(rbl_ctx* ctx, int j, float* out);

/* ---- host-only planning (callable without a GPU) -------------------------------------- */
/* nnz-balanced contiguous row partition: bounds_out[0..nranks] (bounds_out[0]=0). */
int rbl_plan_row_partition(int64_t n, const int64_t* rowptr, int nranks, int64_t* bounds_out);
/* Column footprint of local rows: for each rank q, the contiguous global row range
 * [lo[q],hi[q]) of Q that the local rows reference within q's partition (lo==hi: none). */
int rbl_plan_halo(int64_t nrows_local, const int64_t* rowptr, const int64_t* colind,
                  int index_base, int nranks, const int64_t* bounds, int64_t* lo, int64_t* hi);
/* Hash-window generator on the host (same bits as the device generator): counts only
 * (rowptr_out, n_rows+1) when colind/val are NULL.  Rows [row_begin,row_end). */
int rbl_hashwindow_rows_host(int64_t n, int64_t halfwidth, double density, uint64_t seed,
                             int nplant, const double* plant, int64_t row_begin,
                             int64_t row_end, int64_t* rowptr_out, int64_t* colind_out,
                             double* val_out);
/* The fit rule of RBL_OPT_UPD32_SHADOW: 1 when a shadow of needed_bytes may be allocated on a
 * device that reports free_bytes of total_bytes free (hipMemGetInfo, after the basis and the run's
 * other buffers): it fits and a tenth of the device stays free.  Never changes the basis plan. */
int rbl_plan_shadow_fits(uint64_t free_bytes, uint64_t total_bytes, uint64_t needed_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RBL_HIP_H */
