/* lightkrylov_hip.h -- C ABI of the MI355X-native Krylov inner-loop engine.
 *
 * This is the drop-in boundary for LightKrylov's hot path: everything the reference's
 * Krylov layer (src/Krylov, src/IterativeSolvers) asks of a vector type goes through the
 * six deferred type-bound procedures of `abstract_vector_{rdp,cdp}` and the helpers built
 * on them.  Each entry point below names the reference interface it replaces
 * (file:line under the LightKrylov source tree).  Plain pointers and sizes only: a
 * Fortran `bind(C)` interface block (fortran/lk_hip_iso_c.f90), a ctypes stub
 * (lightkrylov_amd/_capi.py) or C code can bind it as is.
 *
 * Model
 *   - one context per process = one GPU (HIP device + stream).  Multi-GPU = one process
 *     per GPU, each holding a contiguous ROW BLOCK of every vector; the only coupling is
 *     the sum-reduction of dot/norm/projection coefficients, delivered through a
 *     user-installed all-reduce callback (RCCL in production).
 *   - a Krylov basis is ONE column-contiguous panel in HBM: element (i, j) lives at
 *     data[j * ld + i]; ld is padded so every column starts 256-byte aligned.
 *     A single vector is a 1-column basis; every vector argument is a (basis, column) pair
 *     with 0-based column indices.
 *   - "the same memory" is judged by DEVICE ADDRESS, never by handle: a second handle onto a panel
 *     (lk_basis_wrap at the address of one of its columns: a view) names the same columns.  A column
 *     owns the bytes of its rows [0, n_local) and nothing else; two column sets OVERLAP when a column
 *     of the one meets a column of the other, in whole or in part.  The padding rows [n_local, ld)
 *     belong to nobody: another panel may live in them.  A call that writes refuses (LK_ERR_INVALID,
 *     nothing written) an output that overlaps an input it still reads; the exact same column is
 *     the in-place case where an entry has one (lk_vec_axpby, lk_vec_copy's no-op).  Calls that only
 *     read (lk_vec_dot, lk_innerprod, lk_gram) take any overlap.
 *   - dtype LK_F64  = real(dp)     (reference kind "rdp")
 *           LK_C128 = complex(dp)  (reference kind "cdp"), interleaved (re, im).
 *     Scalars cross the ABI as `const double*` to 1 (F64) or 2 (C128) doubles.
 *   - every call returns LK_OK (0) or a negative error code; lk_last_error() gives the text
 *     (the Fortran shim maps non-zero to LightKrylov's stop_error,
 *     src/Utilities/Logger.f90:290-298).  `info` out-arguments follow the reference
 *     convention (src/Krylov/BaseKrylov.fypp:106-109): 0 ok, >0 informational, <0 failure.
 *   - calls are asynchronous on the context's stream except those that return host
 *     scalars, which synchronise that stream once.
 *   There is NO CPU fallback: without a HIP device lk_init fails.
 */
#ifndef LIGHTKRYLOV_HIP_H
#define LIGHTKRYLOV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lk_context_s *lk_context_t;
typedef struct lk_basis_s *lk_basis_t;
typedef struct lk_linop_s *lk_linop_t;

enum { LK_F64 = 0, LK_C128 = 1 };

enum {
    LK_OK = 0,
    LK_ERR_INVALID = -1, /* bad argument / shape / dtype mismatch (reference: stop_error) */
    LK_ERR_HIP = -2,     /* HIP runtime error */
    LK_ERR_NOMEM = -3,
    LK_ERR_COMM = -4,    /* all-reduce callback failed */
    LK_ERR_NAN = -5      /* |beta| = NaN detected (src/Krylov/qr.fypp:137-143) */
};

/* lk_dgs flags */
enum {
    LK_DGS_NORMALIZE = 1 /* fold qr_no_pivoting's 1-column normalise (qr.fypp:134,164) into the call:
                            y <- y / ||y|| on the device when ||y|| >= atol_dp */
};

/* matvec transposition selector for lk_linop_apply (AbstractLinops.fypp:391-424) */
enum { LK_OP_N = 0, LK_OP_H = 1 };

/* ---- context ------------------------------------------------------------------------- */

/* Sum all-reduce over the ranks that share a row-sharded vector: `count` doubles at device
 * address `dev_buf`, in place, ordered on `stream` (a hipStream_t).  Return 0 on success.
 * The reference has no collective at all (reductions are "the user's job inside dot",
 * paper/paper.md:35,97,101); this hook is where that job is done once per sweep. */
typedef int (*lk_allreduce_fn)(void *user, void *dev_buf, int64_t count, void *stream);

int lk_version(void);
const char *lk_last_error(void);

/* device: HIP device ordinal.  stream: a hipStream_t to run on, or NULL for a stream owned
 * by the context. */
int lk_init(int device, void *stream, lk_context_t *ctx);
int lk_finalize(lk_context_t ctx);
int lk_sync(lk_context_t ctx);
int lk_set_allreduce(lk_context_t ctx, lk_allreduce_fn fn, void *user, int nranks, int rank);
/* device ordinal and hipStream_t the context runs on (either pointer may be NULL). */
int lk_context_info(lk_context_t ctx, int *device, void **stream);
/* ranks sharing the row-sharded basis and this context's rank, as installed by lk_set_allreduce or lk_comm_init_rank (1, 0 without
 * either; either pointer may be NULL).  What a host-side check of a row partition must read -- not a shadow of its own. */
int lk_comm_info(lk_context_t ctx, int *nranks, int *rank);

/* Native RCCL all-reduce (one process per GPU; backend "nccl" of the reference-side launchers IS RCCL on
 * ROCm).  Rank 0 calls lk_comm_get_unique_id and ships the LK_COMM_ID_BYTES opaque bytes to every rank by
 * whatever out-of-band channel the host program has (MPI_Bcast in a Fortran/MPI host, the torch.distributed
 * store in bench.py); every rank then calls lk_comm_init_rank (collective: ncclCommInitRank on the context's
 * device), which installs ncclAllReduce(ncclDouble, ncclSum) on the context's stream as the engine's
 * reduction hook -- the <= 129 (258 complex) scalars of each sweep are reduced in place in device memory.
 * The reference itself has no collective (paper/paper.md:35,97,101: "the user's job inside dot").
 * librccl is dlopen'ed on first use.  lk_comm_destroy (or lk_finalize) releases the communicator.
 * lk_comm_available is the LOCAL half of that (no collective, no GPU work): LK_OK when librccl and every entry point the
 * communicator needs resolve in this process -- so that the ranks of a job can agree on the route (native, or a host-provided
 * lk_set_allreduce) BEFORE anyone enters the collective lk_comm_init_rank, where a rank that fails alone leaves the others
 * waiting in the bootstrap (bench.py: the flag is all-reduced over the launcher's process group). */
#define LK_COMM_ID_BYTES 128
int lk_comm_available(void);
int lk_comm_get_unique_id(void *id_out);
int lk_comm_init_rank(lk_context_t ctx, int nranks, int rank, const void *id);
int lk_comm_destroy(lk_context_t ctx);

/* Nearest-neighbour exchange between consecutive ranks of the row partition, needed only by stencil operators
 * (5-point Laplacian: one grid line; Ginzburg-Landau: one point): `count` doubles at device address send_lo go to
 * rank-1 and send_hi to rank+1; recv_lo is filled with rank-1's send_hi, recv_hi with rank+1's send_lo; a NULL pair
 * means "no neighbour on that side".  Ordered on `stream`.  lk_comm_init_rank installs the native one
 * (ncclSend / ncclRecv in one group); lk_set_halo_exchange lets a host bring its own (MPI_Sendrecv, tests). */
typedef int (*lk_halo_fn)(void *user, const void *send_lo, const void *send_hi, void *recv_lo, void *recv_hi,
                          int64_t count, void *stream);
int lk_set_halo_exchange(lk_context_t ctx, lk_halo_fn fn, void *user);

/* All-gather of row blocks, needed only by the row-sharded dense and CSR operators (their matvec needs the whole input
 * vector): rank r contributes counts[r] doubles -- this rank's at device address `send` --, and on return the device buffer
 * `recv` holds every rank's block, rank r's at recv + displs[r] (doubles).  Ordered on `stream`.  lk_comm_init_rank
 * installs the native one (ncclAllGather for equal blocks, else ncclSend / ncclRecv in one group); lk_set_allgather lets a host
 * bring its own (MPI_Allgatherv, tests). */
typedef int (*lk_allgather_fn)(void *user, const void *send, void *recv, const int64_t *counts, const int64_t *displs,
                               int nranks, void *stream);
int lk_set_allgather(lk_context_t ctx, lk_allgather_fn fn, void *user);

/* row block owned by this rank: global rows [row0, row0 + n_local) of n_global; only used
 * so that counter-based rand fills are identical for every partition. */
int lk_set_partition(lk_context_t ctx, int64_t row0, int64_t n_global);
/* Tuning keys (integers; 30 of them -- round 6 removed every key whose other setting was measured slower and never defaulted, the
 * record of those A/Bs is docs/TUNING_LOG.md).  None changes a result beyond rounding; the ones marked [bits] change no result bit.
 *   schedule      "async_arnoldi" (1: lk_arnoldi / lk_arnoldi_block enqueue all steps behind a device-side breakdown flag, one host
 *                 synchronisation per call; 0: one round trip per step; lk_lanczos / lk_bidiag always enqueue and do not read the key)
 *                 [bits]; "lazy", "lazy_speculate" (see lk_lazy_stats) [bits];
 *                 "pool_slab_cols" (columns per pool slab) [bits]
 *                 "fuse_rowop" (the asynchronous lk_arnoldi batch on a diagonal operator -- lk_linop_diag_create, lk_linop_diag_linspace.
 *                 0: the operator kernel writes y first.  1: no operator kernel: the three sweeps form y = D x_k from column k-1 of the
 *                 panel as they stream it, y never exists in memory, 3k + 3 columns per step instead of 3k + 8; same product, same
 *                 summation order as 0 [bits].  2 [default]: as 1, and on a context without a communicator, real kind, panels of at
 *                 least 8 runs per CU ("stream_two"'s size rule: 1.68e7 rows on 256 CUs), sweep 3 of a step also forms h1 and ||y||^2
 *                 of the NEXT step from y'' in its registers, so that step runs no sweep 1: two passes over the basis per step, 2k + 2
 *                 columns.  h1 of steps 2.. is then (sum x (d y'')) / beta where 1 forms sum x (d (y'' / beta)): H and the basis move in
 *                 the last bits, and a factorisation made in several calls (each call's first step runs a sweep 1) differs in the last
 *                 bits from one call.  3: as 2 at every size)
 *   single launch "resident", "resident_max_mb", "resident_onchip", "resident_rev", "resident_spin_ms" (see lk_resident_stats)
 *   sweeps        "recompute_update" (1: sweep 2 keeps y' in registers, sweep 3 re-forms it: y' never goes to HBM; 0: y' stored, sweep 3
 *                 on the streaming update kernel -- another summation order over the columns, so y'' changes by rounding); "store_policy"
 *                 (cache policy of the sweeps' 16-byte y store: 0 plain, 1 nt, 2 sc1 = write-through [default], 3 sc0 sc1) and
 *                 "store_split" [bits]; "stream_two" (sweep 3 of the recomputing schedule against at most 128 columns one column at a time,
 *                 y in registers and y'' stored once per run of rows, in sweep 2's summation order: y'' bit for bit as the tile kernel
 *                 writes it, its norm summed over another row-to-lane mapping and so equal by rounding only; 1 = always, 2 = the real
 *                 kind on long panels, 0 = the tile kernel); "dot_colwise" (1: sweep 1 / innerprod one column at a time, panel_dot_cw; 0: all columns per
 *                 tile) with "cw_u" (16-byte loads per lane and column: 4, 8, 0 = by size) and "cw_grid_mult"; "grid_mult", "blas1_grid_mult" (blocks per CU: the number of per-block partial sums a dot is assembled from);
 *                 "wide_regs" (update sweeps against 129..384 columns: 2 = register tiles of 32 / 24 columns + the lane split on 24-column
 *                 groups, 1 = the first only, 0 = lane split on 16-column groups) and "wide_s3" (1: sweep 3 of a lane-split step holds both
 *                 column groups of a wave-column in one wave's registers) [bits]
 *   matrix cores  "xhy_mfma" (1: X^H Y with five or more right-hand sides -- Gram, innerprod_matrix, block Gram-Schmidt -- in one pass over
 *                 X on the FP64 MFMAs; 0: four right-hand sides per pass on the vector units); "block_fused" (block Gram-Schmidt: 1 = three
 *                 passes per group for the real kind, 2 = for both kinds, 0 = four); "gemm_mfma_min" (tall-skinny product on the MFMAs from
 *                 this many output columns on; default 5 real / 9 complex); "gemm_3m" (1: the complex MFMA kernels use three real products
 *                 per complex one); "xhy_db" (panel_xhy_mfma with a double-buffered LDS tile: 1 = the 128-column variants, 2 = all, 0 = never); "gemm_roll" (1: the real product with 33..64 outputs keeps a ring of four k-steps of X in flight; 2:
 *                 every variant that has a ring; 0: batches) [bits]; "gram_rs" (Gram matrix of 5..128 real columns by panel_gram_rs and of 5..112
 *                 complex columns by panel_gram_rs3m / panel_gram_rs3m4 -- rows of the staged tile dealt to the waves, tiles staged by LDS-DMA: 1 = the resident
 *                 number of blocks per CU, n > 1 = n blocks per CU, 0 = panel_xhy_mfma / panel_gram_mfma3m); "upd_rs" (fused pass of the block Gram-Schmidt, real kind, 17..32 right-hand sides: 1 = panel_xhy_upd_rs --
 *                 row-owner waves on LDS-DMA tiles, coefficients in registers --, 0 = panel_xhy_upd_mfma)
 *   operators     "csr_stream" (1: CSR product through LDS for matrices with short rows; 0: lanes-per-row kernel)
 * A build made with -DLK_DIAGNOSTICS (make -C lightkrylov_amd/csrc diagnostics; NOT what build() produces) adds "xhy_debug" / "upd_debug",
 * which switch parts of a kernel off for phase timing and give WRONG results; the shipped library rejects them as unknown keys. */
int lk_set_tuning(lk_context_t ctx, const char *key, int value);

/* Lazy batching of the per-object path (tuning key "lazy", off by default).  When on, k consecutive
 * lk_vec_dot(X, j, y) calls over the columns of one panel cost ONE sweep (the first call computes the whole
 * run, the rest are memo hits) and consecutive lk_vec_axpby(a_j, X, j, 1, y) calls are queued and applied as
 * ONE panel update when anything else touches the engine.  This is what turns the schedule an unchanged
 * LightKrylov drives through the type-bound procedures (innerprod / linear_combination loops,
 * AbstractVectors.fypp:672-674, 600-602) into fused traffic.  out4 = {dot memo hits, batched dot sweeps,
 * queued axpbys, queue flushes}. */
int lk_lazy_stats(lk_context_t ctx, int64_t *out4);
/* The temporary of linear_combination (AbstractVectors.fypp:595-603: `allocate(y, source=X(1)); y%zero(); y%axpby(..)`)
 * stays VIRTUAL in lazy mode: its zero() and its k axpbys are recorded, the `y%sub(proj)` that consumes it
 * (gram_schmidt.fypp:145) becomes a pending y -= X h, and the NEXT pass's `y%norm()` (gram_schmidt.fypp:126, qr.fypp:135)
 * runs one sweep that forms and stores y', and returns ||y'|| and X^H y' for the k dot calls that follow: ONE pass over
 * X per Gram-Schmidt pass, 3k+6 columns per double_gram_schmidt_step against 3k+4 for lk_dgs.  The temporary is
 * written only if something reads it.  out4 = {fused update+dot sweeps, pending updates applied as plain panel updates,
 * virtual temporaries dropped unwritten, virtual temporaries written after all}. */
int lk_lazy_fusion_stats(lk_context_t ctx, int64_t *out4);
/* The first pass of a Gram-Schmidt step opens with y%norm() and then asks X(1..k)%dot(y) (gram_schmidt.fypp:126, 141): a norm
 * kernel and the batched dot sweep, two host synchronisations -- although the sweep computes ||y||^2 on the side.  Once that pair
 * has been seen for y = column j of a panel, the norm of column j + 1 (the next Arnoldi / Lanczos step) runs the sweep at once and
 * serves the norm and the k dots from it (tuning key "lazy_speculate", default 1).  A prediction nobody uses disarms it.
 * out2 = {anticipated sweeps, of which unused}. */
int lk_lazy_speculation_stats(lk_context_t ctx, int64_t *out2);

/* Single-launch Gram-Schmidt step (round 6; csrc/lk_resident.hip.h).  When the panel X(:, :k) | y fits the 256 MB memory-side
 * cache -- the launch-bound regime of the reference's own use cases (1.75 10^5 unknowns, paper/paper.md:103-113) -- lk_dgs and every
 * step of lk_arnoldi run double_gram_schmidt_step (gram_schmidt.fypp:12-57) AND qr_no_pivoting's norm + scale (qr.fypp:135-165) as ONE
 * persistent kernel: each block keeps its rows for the three phases, the phases' sums meet inside the launch in a fixed order.  Panels
 * up to the register files' capacity (64 MB on the chip) stay IN REGISTERS for the whole step: X is read once, k + 2 columns of
 * traffic instead of 3k + 5.  Tuning keys: "resident" (default 1; 0 = always the three-sweep schedule), "resident_max_mb" (default 320:
 * MB of panel the single launch takes), "resident_onchip" (default 1; 0 = never the register-resident kernel), "resident_rev" (tile
 * order of the cache-resident kernel's phase 2) and "resident_spin_ms" (default 50: bound on the first grid-wide wait, which normally ends within microseconds -- 0 = give up there at
 * once, the tests' way to the fallback --; a launch that cannot get all its blocks on the chip, e.g. because another context's persistent
 * kernel holds part of it, gives up BEFORE writing anything, that step runs on the three-sweep schedule, and the single launch pauses for 16
 * steps -- doubling with every further give-up -- before it is tried again; setting "resident" = 1 re-arms it at once).  One rank only: a row-sharded context keeps the three launches, whose sums meet in the all-reduce.  Same
 * results to rounding (different summation order).
 * out3 = {single launches enqueued, launches that gave up, launches that kept the panel in registers}. */
int lk_resident_stats(lk_context_t ctx, int64_t *out3);
/* In-kernel timeline of the LAST single launch (profiling aid, like lk_profile_get): the 100 MHz wall clock of block 0 at
 * kernel entry | phase 1 done (the panel read included) | sum 1 done | phase 2 done | sum 2 done | phase 3 done | sum 3 done | scaled.  Synchronises the stream. */
int lk_resident_phase_ticks(lk_context_t ctx, int64_t *out8);

/* per-kernel HIP-event timing on the context's stream (bench.py roofline leg).
 * tags: "dgs_sweep1|2|3" (the three panel sweeps; "dgs_sweep*" sums them -- a trailing '*' is a
 * prefix match), "dgs" (whole lk_dgs call), "matvec", "blas1". */
int lk_profile_enable(lk_context_t ctx, int on);
int lk_profile_get(lk_context_t ctx, const char *tag, int64_t *count, double *total_ms,
                   double *total_bytes);
int lk_profile_reset(lk_context_t ctx);

/* ---- basis = array of vectors, X(:) in the reference --------------------------------- */

/* replaces `allocate(X(ncols), source=...)` + `zero_basis(X)` (AbstractVectors.fypp:711-715,
 * IterativeSolvers.fypp:1032-1034): n_local rows on this rank, columns zero-filled. */
int lk_basis_create(lk_context_t ctx, int dtype, int64_t n_local, int ncols, lk_basis_t *B);
/* wrap caller-owned device memory (e.g. a torch tensor).  ld in elements; dev_ptr 16-byte
 * aligned; ld even for LK_F64.  Rows [n_local, ld) are never read or written.  This is also how
 * a VIEW of columns [j, j + ncols) of a panel is made (same ld, dev_ptr = the address of column j):
 * every entry treats view and parent as the same memory (the overlap rule under "Model"). */
int lk_basis_wrap(lk_context_t ctx, int dtype, int64_t n_local, int ncols, int64_t ld,
                  void *dev_ptr, lk_basis_t *B);
int lk_basis_destroy(lk_basis_t B);
/* shape and base address of the panel.  The address is for building views (lk_basis_wrap) and for memory the caller owns;
 * to READ OR WRITE a vector's contents from a kernel of your own use lk_vec_device_ptr, which first applies what the engine
 * may still owe that vector in lazy mode. */
int lk_basis_info(lk_basis_t B, int *dtype, int64_t *n_local, int *ncols, int64_t *ld,
                  void **dev_ptr);
/* A USER'S OWN KERNEL on a vector (a hand-written `matvec`, AbstractLinops.fypp:74-87): the device address of column j,
 * valid until the vector is released, with everything the engine still owes that vector applied first (lazy mode defers
 * updates).  `access` says what the caller will do: LK_ACCESS_READ, LK_ACCESS_OVERWRITE (previous contents not read:
 * `vec_out` is intent(out)) or LK_ACCESS_READWRITE.  The caller's work must be ordered after the engine's: enqueue it on
 * the context's stream (lk_context_info) or call lk_sync first; n_local elements of the basis' dtype, contiguous. */
#define LK_ACCESS_READ 0
#define LK_ACCESS_OVERWRITE 1
#define LK_ACCESS_READWRITE 2
int lk_vec_device_ptr(lk_basis_t B, int j, int access, void **dev_ptr);
/* host <-> device, `ncols` columns starting at col0; host is column-major with leading
 * dimension ldh (elements).  Synchronous. */
int lk_basis_upload(lk_basis_t B, int col0, int ncols, const void *host, int64_t ldh);
int lk_basis_download(lk_basis_t B, int col0, int ncols, void *host, int64_t ldh);

/* ---- column pool: device storage for hosts that own vectors OBJECT BY OBJECT ---------
 * LightKrylov creates vectors one object at a time, by sourced allocation, polymorphic assignment and
 * intent(out) dummies, and never frees them explicitly (AbstractVectors.fypp:595-598, gmres.fypp:110-115,155;
 * SURVEY 8b "Ownership").  A plugin type therefore cannot own device memory through allocate/final; it asks
 * this pool for a COLUMN of a shared slab (a panel of `pool_slab_cols` columns, tuning key, default 160; a single-rank
 * context takes fewer when that would exceed a quarter of the free memory, a row-sharded one never does -- the slab geometry
 * must be the same on every rank, so there an allocation that does not fit FAILS with LK_ERR_NOMEM) keyed
 * by an owner tag -- the address of the Fortran object:
 *   lk_pool_acquire  returns the column already registered to `owner_tag` (an object that reappears at the
 *                    address of a dead one re-uses its column: temporaries such as linear_combination's `proj`
 *                    cost no new memory per call), else the lowest released column, else the next column of the
 *                    open slab, so `allocate(V(k), source=b); call zero_basis(V)` lands in consecutive columns
 *                    of one panel and the lazy per-object path (lk_lazy_stats) can batch it;
 *   lk_pool_owner    tag a column is registered to (0: free or not a pool column; `slab` is validated
 *                    against the pool before it is dereferenced, so stale handles are safe to ask about);
 *   lk_pool_column_info  the same plus the column's GENERATION: a fresh value of ONE per-context counter that only grows (never
 *                    per slab, never reset by lk_pool_release_all: no value is ever handed out twice), assigned every time
 *                    lk_pool_acquire hands the column out (first use, re-use by tag, re-use after a release).  A plugin stores the generation in its
 *                    handle: a bit copy of a handle whose source object has since died and been replaced at the same address
 *                    (`allocate(b, source=dense_vector_gpu(x))` followed by another temporary) carries an old generation and
 *                    is refused instead of silently reading the new occupant's data;
 *   lk_pool_release  returns one column; lk_pool_release_all destroys every slab (after a solver call);
 *   lk_pool_stats    out4 = {slabs, columns ever carved, columns currently registered, acquisitions served by
 *                    re-use}. */
int lk_pool_acquire(lk_context_t ctx, int dtype, int64_t n_local, uint64_t owner_tag, lk_basis_t *slab,
                    int *col);
int lk_pool_owner(lk_context_t ctx, lk_basis_t slab, int col, uint64_t *owner_tag);
int lk_pool_column_info(lk_context_t ctx, lk_basis_t slab, int col, uint64_t *owner_tag, uint64_t *generation);
int lk_pool_release(lk_context_t ctx, lk_basis_t slab, int col);
int lk_pool_release_all(lk_context_t ctx);
int lk_pool_stats(lk_context_t ctx, int64_t *out4);

/* ---- abstract_vector type-bound procedures (AbstractVectors.fypp:295-381) ------------ */

/* zero(self)                         AbstractVectors.fypp:322-326, dense: 476-486 */
int lk_vec_zero(lk_basis_t B, int j);
/* rand(self, ifnorm)                 AbstractVectors.fypp:328-336, dense: 488-503.  Counter-based generator:
 * entry i (global row row0+i) = 2u-1, u = (splitmix64(seed*2^32 + ctr) >> 11) * 2^-53;
 * ctr = row for F64, 2*row / 2*row+1 for re / im.  ifnorm != 0 normalises (what eigs expects
 * of rand(.true.), IterativeSolvers.fypp:1040). */
int lk_vec_rand(lk_basis_t B, int j, uint64_t seed, int64_t row0, int ifnorm);
/* scal(self, alpha)                  AbstractVectors.fypp:338-344, dense: 505-512 */
int lk_vec_scal(lk_basis_t B, int j, const double *alpha);
/* axpby(alpha, vec, beta, self): self <- alpha*vec + beta*self   AbstractVectors.fypp:346-356,
 * dense: 514-536.
 * True axpby in ONE pass (the reference's dense version does scal-then-axpy). */
int lk_vec_axpby(const double *alpha, lk_basis_t Bx, int jx, const double *beta, lk_basis_t By,
                 int jy);
/* dot(self, vec) = sum conj(self) * vec, all-reduced over ranks.
 * AbstractVectors.fypp:358-365, dense: 538-555.
 * out: 1 or 2 doubles. */
int lk_vec_dot(lk_basis_t Bx, int jx, lk_basis_t By, int jy, double *out);
/* norm(self) = sqrt(abs(dot(self,self)))   AbstractVectors.fypp:424-432 */
int lk_vec_norm(lk_basis_t B, int j, double *out);
/* get_size(self): GLOBAL size is the caller's business; this returns the local row count.
 * AbstractVectors.fypp:367-372 */
int lk_vec_size(lk_basis_t B, int64_t *n_local);
/* copy(out, from)                    AbstractVectors.fypp:717-723 */
int lk_vec_copy(lk_basis_t Bdst, int jd, lk_basis_t Bsrc, int js);

/* ---- basis helpers built on the TBPs (cannot be specialised by a Fortran plugin; here
 *      they are fused panel kernels) ---------------------------------------------------- */

/* innerprod(X(:k), Y(jy0:jy0+p)) -> M = X^H Y, k x p column-major on the host.
 * AbstractVectors.fypp:659-695 */
int lk_innerprod(lk_basis_t Bx, int k, lk_basis_t By, int jy0, int p, double *M);
/* linear_combination(Y, X(:k), B): Y(:, jy0+j) = X(:, :k) * C(:, j), C is k x q column-major
 * on the host.  AbstractVectors.fypp:571-643 */
int lk_lincomb(lk_basis_t Bx, int k, const double *C, int q, lk_basis_t By, int jy0);
/* Gram(X(:k)) -> G k x k (upper computed, mirrored without conjugation like the reference).
 * AbstractVectors.fypp:645-657 */
int lk_gram(lk_basis_t Bx, int k, double *G);
/* orthogonalize_against_basis(y, X(:k), info, beta=h): ONE classical Gram-Schmidt pass.
 * src/Krylov/gram_schmidt.fypp:113-154.  h: k scalars on the host (may be NULL). */
int lk_orthogonalize(lk_basis_t Bx, int k, lk_basis_t By, int jy, double *h, int *info);
/* double_gram_schmidt_step(y, X(:k), info, if_chk_orthonormal=.false., beta=h)
 * src/Krylov/gram_schmidt.fypp:12-57; interface src/Krylov/BaseKrylov.fypp:634-712.
 * Three fused panel sweeps (h1 = X^H y | y' = y - X h1, h2 = X^H y' | y'' = y' - X h2) for k <= 512 basis columns: 3k+4
 * columns of traffic (129..512 columns: the lanes of a wave are split over column groups so that a block still holds all k
 * columns of its tile); 513..2048 columns run as column panels of 512 on the device (4k - |last panel| columns, one host
 * synchronisation), wider bases panel by panel with a host round trip each.
 * h = h1 + h2 on the host (k scalars, may be NULL).
 * norms[0..2] = ||y||, ||y'||, ||y''|| (may be NULL).  info = 1 when ||y'|| < atol_dp (the
 * reference's pass-2 zero-vector flag, gram_schmidt.fypp:126-127), else 0. */
int lk_dgs(lk_basis_t Bx, int k, lk_basis_t By, int jy, double *h, double *norms, int flags,
           int *info);
/* basis-against-basis variant (gram_schmidt.fypp:59-105): Y(jy0:jy0+p) against X(:k),
 * h is k x p column-major.  Panel x panel schedules for k <= 128 -- p <= 4: the fused sweeps with several right-hand sides
 * (three passes over X per group of <= 2 columns, or of 4 columns of the real kind for k <= 64; else four);  p >= 5: the
 * coefficients and updates on the FP64 matrix cores, per group of <= 32 columns H1 = X^H Y | Y' = Y - X H1 with H2 = X^H Y' in the
 * same pass | Y'' = Y' - X H2: THREE passes over X (real kind; the complex kind keeps four: H1 | update | H2 | update).
 * Wider bases: column by column through lk_dgs. */
int lk_dgs_block(lk_basis_t Bx, int k, lk_basis_t By, int jy0, int p, double *h, int *info);

/* ---- operators (stand where a user's abstract_linop matvec/rmatvec stands,
 *      AbstractLinops.fypp:58-87); synthetic drivers of the path ------------------------ */

/* y = d .* x; d: n_local host values of the basis dtype. */
int lk_linop_diag_create(lk_context_t ctx, int dtype, int64_t n_local, const void *d_host,
                         lk_linop_t *op);
/* d_i = d0 + dstep * (row0 + i), generated on the device (F64 only). */
int lk_linop_diag_linspace_create(lk_context_t ctx, int64_t n_local, int64_t row0, double d0,
                                  double dstep, lk_linop_t *op);
/* dense_linop: y = A x ('N') or A^H x ('H'); A is n x n column-major on the host.
 * AbstractLinops.fypp:265-271, 608-660.  Whole matrix on one rank (row-sharded: the _sharded variants below). */
int lk_linop_dense_create(lk_context_t ctx, int dtype, int64_t n, const void *A_host, int64_t lda,
                          lk_linop_t *op);
/* row-sharded dense_linop ("row block of A + allgather of x"): rank r owns rows [row_starts[r], row_starts[r+1]) of
 * the n_global x n_global matrix and of every vector (row_starts: nranks + 1 entries, the same on every rank; the context's
 * rank picks the block).  A_rows: this rank's n_local x n_global block, column-major, leading dimension lda >= n_local.
 *   matvec  : x is all-gathered over the ranks (lk_allgather_fn), y_local = A_rows x -- the same products and the same
 *             summation order per row as the single-rank operator;
 *   rmatvec : z = A_rows^H x_local has n_global entries on every rank; their sum over the ranks (the all-reduce hook) is A^H x,
 *             of which each rank keeps its rows (to rounding: the single-rank operator sums a column in one piece).
 * _wrap_ takes the block where it already lies in DEVICE memory (16-byte aligned, lda even for LK_F64; not copied, not freed). */
int lk_linop_dense_create_sharded(lk_context_t ctx, int dtype, int64_t n_global, const int64_t *row_starts, const void *A_rows,
                                  int64_t lda, lk_linop_t *op);
int lk_linop_dense_wrap_sharded(lk_context_t ctx, int dtype, int64_t n_global, const int64_t *row_starts, void *dev_ptr,
                                int64_t lda, lk_linop_t *op);
/* sparse operator in CSR: y = A x ('N') or A^H x ('H'), A n x n, 0-based `rowptr[n+1]` / `colind[nnz]`, values of
 * `dtype` -- a user's sparse `abstract_linop` (AbstractLinops.fypp:58-87; the reference has no sparse type of its own:
 * its Poisson / Ginzburg-Landau examples write the stencil by hand).  The arrays are copied; A^H is built once on the
 * host so that rmatvec is a row-parallel product too.  Whole matrix on one rank (row-sharded: below). */
int lk_linop_csr_create(lk_context_t ctx, int dtype, int64_t n, const int64_t *rowptr, const int32_t *colind,
                        const void *vals, lk_linop_t *op);
/* row-sharded CSR operator: rank r owns rows [row_starts[r], row_starts[r+1]); rowptr (n_local + 1 entries, 0-based) / colind /
 * vals describe those rows with GLOBAL column indices.  COLLECTIVE: every rank calls it at the same point (the ranks exchange
 * which entries of x their rows reference, through the all-gather hook).  matvec then moves only THOSE entries -- each rank packs
 * what others need of its block, the packed pieces are all-gathered, the local rows multiply [own rows | pieces]: a stencil or
 * banded matrix exchanges a few boundary entries per neighbour, not x -- unless half of x or more would travel anyway, in which
 * case x is all-gathered whole as for the dense operator.  Either way a row's entries are summed in the same order as on one rank.
 * rmatvec sums the ranks' full-length products of their blocks' conjugate transposes (all-reduce hook) and keeps the local rows.
 * Errors are collective too: the validation of a rank's row block (column index out of range, decreasing rowptr, null arrays),
 * its buffer allocations and its uploads are each AGREED ON through the same hook before the next exchange, so when any rank fails
 * every rank returns an error and no operator (the failing rank its own message, the others "rank r failed") -- nobody is left
 * waiting in an exchange.  The one exception: a rank that cannot allocate the staging buffers of the metadata exchange itself
 * (P-length tables, the request lists) returns alone; that is fatal for the job. */
int lk_linop_csr_create_sharded(lk_context_t ctx, int dtype, int64_t n_global, const int64_t *row_starts, const int64_t *rowptr,
                                const int32_t *colind, const void *vals, lk_linop_t *op);
/* 5-point Laplacian on an N x N grid, Dirichlet, scaled by (N+1)^2 (BASELINE config 3).
 * F64; whole grid on one rank (row-sharded: the _sharded variant below). */
int lk_linop_lap5_create(lk_context_t ctx, int64_t N, lk_linop_t *op);
/* row-sharded: this rank owns grid lines [j0, j0 + nj), i.e. vector rows [j0*N, (j0+nj)*N); the neighbouring
 * ranks' boundary lines arrive through the halo exchange (one line of N doubles each way per application). */
int lk_linop_lap5_create_sharded(lk_context_t ctx, int64_t N, int64_t j0, int64_t nj, lk_linop_t *op);
/* Exponential-propagator stand-in of the Ginzburg-Landau example (BASELINE config 4): y = Phi_tau x,
 * Phi_tau = `nsub` classical RK4 steps of the linearised complex GL right-hand side with the reference's
 * stencil and boundary rows (example/ginzburg_landau/Ginzburg_Landau.f90:126-136; LK_OP_H uses the adjoint
 * right-hand side, :170-179).  x_i = -L/2 + i*dx, L = dx*(n+1); mu_i = mu_c + (mu2/2) x_i^2.
 * nu, gamma: 2 doubles each.  LK_C128; whole domain on one rank (row-sharded: the _sharded variant).  (The reference integrates with rklib's adaptive
 * rks54, an un-vendored dependency; a fixed-step RK4 is used by oracle and engine alike.) */
int lk_linop_gl_create(lk_context_t ctx, int64_t n, double dx, double tau, int nsub, const double *nu,
                       const double *gamma, double mu_c, double mu2, lk_linop_t *op);
/* row-sharded: this rank owns rows [row0, row0 + n_local) of n_global; every RK4 stage exchanges one point with each
 * neighbouring rank through the halo exchange. */
int lk_linop_gl_create_sharded(lk_context_t ctx, int64_t n_global, int64_t row0, int64_t n_local, double dx,
                               double tau, int nsub, const double *nu, const double *gamma, double mu_c,
                               double mu2, lk_linop_t *op);
/* Product of two engine operators: LK_OP_N applies y = op_a(A) op_b(B) x, LK_OP_H the adjoint op_b(B)^H op_a(A)^H x (transA / transB:
 * LK_OP_N or LK_OP_H) -- what a user's abstract_linop whose matvec chains two others does (AbstractLinops.fypp:58-87), and how a fixed
 * right preconditioner enters an Arnoldi batch without a host round trip (gmres.fypp:155-165: V(k+1) = A M V(k)).  The operator owns ONE
 * scratch vector, allocated here; its application enqueues the two factors' through it -- the same kernels, the same bits as two
 * lk_linop_apply calls through a temporary -- so it works on a row-sharded context whenever both factors do.  It does NOT own A or B:
 * both must outlive it.  No row-local form (the "fuse_rowop" schedules do not apply); its "matvec" bytes are the factors' plus the
 * scratch written and read.  lk_arnoldi, lk_kexpm and eigs on a product of engine operators run fused through it.
 * LK_ERR_INVALID: a null argument; factors of different context, kind or size. */
int lk_linop_compose_create(lk_linop_t A, int transA, lk_linop_t B, int transB, lk_linop_t *op);
int lk_linop_destroy(lk_linop_t op);
/* apply_matvec / apply_rmatvec: y(:, jy) = op(A) x(:, jx).  AbstractLinops.fypp:391-424 */
int lk_linop_apply(lk_linop_t op, int trans, lk_basis_t Bx, int jx, lk_basis_t By, int jy);
/* r = b - op(A) x and ||r||: gmres.fypp:134-142 (and :205-214; CG.fypp:108-109), which spell it matvec, sub, chsgn, norm.  The
 * operator's product is enqueued into r, then ONE kernel (k_axpby's residual branch) forms r <- b - r in place and the per-block sums
 * of |r|^2 in the same pass
 * (finished in a fixed order, no floating-point atomics; all-reduced over the ranks of a row-sharded context): one read-write pass
 * where sub, chsgn and norm take two and a read pass.  r is bit for bit what the three calls leave; the norm agrees to rounding
 * (another summation order).  nrm may be NULL: the sum then stays on the device and the call does not synchronise.
 * LK_ERR_INVALID: r the same column as x or b; operator and vectors of different shape, kind or context.  A NaN is no error here:
 * it comes back as the norm. */
int lk_linop_residual(lk_linop_t A, int trans, lk_basis_t Bx, int jx, lk_basis_t Bb, int jb, lk_basis_t Br, int jr, double *nrm);

/* ---- the caller of the path: Arnoldi --------------------------------------------------
 * arnoldi(A, X, H, info, kstart, kend, tol, transpose) with blksize = 1 (lk_arnoldi_block: any blksize).
 * src/Krylov/arnoldi.fypp:8-76 (+ the 1-column qr_no_pivoting, src/Krylov/qr.fypp:116-167).
 * X: basis with m+1 columns; H: host (ldh x m) column-major array of the basis dtype;
 * kstart/kend 1-based inclusive; tol: breakdown tolerance (reference default atol_dp).
 * info = 0, or k when |H(k+1,k)| < tol (invariant subspace, loop exits).  Steps up to 512 basis columns are enqueued
 * asynchronously (one host synchronisation per call); beyond that one round trip per step. */
int lk_arnoldi(lk_linop_t A, lk_basis_t X, double *H, int64_t ldh, int kstart, int kend,
               double tol, int trans, int *info);
/* The same factorisation (same bits), delivered IN SEGMENTS while it runs: the steps are enqueued back to back as one asynchronous batch,
 * and as soon as the device has produced the steps up to seg_last[i] (nseg ascending step numbers within [kstart, kend]) their columns of H
 * are written and fn(user, kfirst, klast) is called on the calling thread -- while the later steps are still running on the device.  The
 * per-step host work of a caller overlaps the rest of the call with no idle gap on the device between segments: eigs tests the Ritz pairs of
 * H(1:k, 1:k) after every step (src/IterativeSolvers/IterativeSolvers.fypp:1059-1093); one blocking lk_arnoldi call per segment cost its
 * Krylov-Schur cycle ~0.4 ms of device idling per boundary.  fn is called for every step range exactly once, in order, the last time
 * before the call returns; columns beyond a breakdown are never reported.  fn returns 0 to go on, non-zero to STOP: nothing more is
 * enqueued (the device is kept at most 24 steps ahead of the segment being delivered, so at most that many steps beyond the last
 * reported one have touched the basis), nothing more is reported, and the call returns with info = 0 (eigs stops a cycle at the first
 * step with enough converged pairs, :1087-1093).  fn must not call into the same context.  fn may be NULL (then this is lk_arnoldi).
 * ROW-SHARDED CONTEXTS (nranks > 1): every step carries three all-reduces, and each rank stops enqueueing where ITS fn says so -- the
 * library has no agreement step here (one more collective per delivery would drain the 24 steps of lookahead this entry exists for).
 * So the value fn returns for a given (kfirst, klast) must be THE SAME ON EVERY RANK: a function of H (identical on all ranks after the
 * all-reduce) is; wall-clock time, or state set asynchronously by another thread, is not -- ranks that stop at different steps leave
 * unmatched collectives behind (a hang, or sums paired across steps).  The mirror's eigs never asks a sharded cycle to stop early. */
typedef int (*lk_progress_fn)(void *user, int kfirst, int klast);
int lk_arnoldi_segments(lk_linop_t A, lk_basis_t X, double *H, int64_t ldh, int kstart, int kend, double tol, int trans,
                        const int *seg_last, int nseg, lk_progress_fn fn, void *user, int *info);

/* ---- Lanczos tridiagonalisation (symmetric / Hermitian operators) ------------------------
 * lanczos_tridiagonalization(A, X, T, info, kstart, kend, tol): src/Krylov/lanczos.fypp:7-64.
 * Per step: X(k+1) = A X(k); T(i, k) = X(i)%dot(X(k+1)), X(k+1) -= T(i, k) X(i) for i = max(1, k-1), k (:57-60); full
 * re-orthogonalisation by a double Gram-Schmidt step without beta (:62); T(k+1, k) = ||X(k+1)||; beta < tol => info = k and
 * the loop exits WITHOUT scaling (:32-36), else X(k+1) is normalised.  All steps of a call are enqueued asynchronously
 * (device-side stop flag), one host synchronisation per call.  T: host (ldt x m) column-major array of the basis dtype;
 * only T(k-1:k+1, k) of each step is written.  Steps against more than 512 basis columns run one host round trip each (the reference has no
 * cap, lanczos.fypp:20). */
int lk_lanczos(lk_linop_t A, lk_basis_t X, double *T, int64_t ldt, int kstart, int kend, double tol, int *info);

/* ---- Golub-Kahan bidiagonalisation -----------------------------------------------------------
 * lanczos_bidiagonalization(A, U, V, B, info, kstart, kend, tol): src/Krylov/golub_kahan.fypp:7-64.
 * Per step: V(k) = A^H U(k), double Gram-Schmidt against V(:k-1) (k > 1), B(k, k) = alpha = ||V(k)||, normalise (:27-42);
 * U(k+1) = A V(k), double Gram-Schmidt against U(:k), B(k+1, k) = beta = ||U(k+1)||, normalise (:45-58); a norm not above
 * tol => info = k and the loop exits without scaling.  All steps of a call are enqueued asynchronously (device-side stop flag
 * per half step), one host synchronisation per call.  U: kdim + 1 columns, V: >= kdim columns (two different bases); B: host
 * (ldb x kdim) column-major array of the basis dtype, only B(k, k) and B(k+1, k) are written.  tol >= atol_dp.  Steps against more than
 * 512 basis columns run one host round trip each (the reference has no cap, golub_kahan.fypp:18). */
int lk_bidiag(lk_linop_t A, lk_basis_t U, lk_basis_t V, double *B, int64_t ldb, int kstart, int kend, double tol, int *info);

/* ---- qr_no_pivoting and the block Arnoldi factorisation (round 6) ------------------------------------------
 * qr_no_pivoting(Q, R, info, tol): src/Krylov/qr.fypp:116-167, on columns [j0, j0 + p) of a panel.  Column j: double Gram-Schmidt
 * against the j columns before it with beta = R(:j-1, j) (:131-134), beta = ||q_j|| (:135), NaN aborts (:137-143); beta < tol => info = j
 * (first such column), R(j, j) = 0, the column is re-drawn from the counter generator (stream 0x5EED + panel column + 1), orthogonalised
 * again and its new norm taken (:146-162), else R(j, j) = beta; q_j scaled by 1 / beta (:164).  R: host p x p column-major (leading
 * dimension ldr elements) of the basis dtype, zeroed by the call; rows p..ldr-1 are not touched (the reference's R = zero, :125, covers a
 * larger R as well: the caller clears them).  Host-synchronous, column by column. */
int lk_qr(lk_basis_t Q, int j0, int p, double *R, int64_t ldr, double tol, int *info);
/* arnoldi(A, X, H, info, kstart, kend, tol, transpose, blksize): src/Krylov/arnoldi.fypp:8-76 with blksize = p > 1 (p = 1 is lk_arnoldi).
 * X holds (kdim + 1) p columns (kdim = (ncols - p) / p, :26), H is host ((kdim + 1) p x kdim p), column-major, leading dimension ldh.
 * Step k (kpm = (k-1) p, kp = k p): X(kp + i) = A X(kpm + i) (:39-47), the batch Gram-Schmidt of the new block against X(:kp) into
 * H(:kp, kpm+1:kp) (:50-51, panel x panel on the matrix cores from five columns on), qr_no_pivoting of the block into
 * H(kp+1:kp+p, kpm+1:kp) (:55), min |diagonal| < tol => info = kp, exit (:58-71).  All steps of a call are enqueued asynchronously
 * behind a device-side stop flag that counts (step, column): a column below max(tol, atol_dp) stops everything behind it, the host
 * finishes that block (re-draw, remaining columns) exactly as lk_qr would; ONE copy and ONE host synchronisation per call otherwise.
 * Bases beyond 512 columns, and "async_arnoldi" = 0, run one round trip per step through lk_dgs_block / lk_qr. */
int lk_arnoldi_block(lk_linop_t A, lk_basis_t X, double *H, int64_t ldh, int blksize, int kstart, int kend, double tol, int trans,
                     int *info);

/* ---- matrix exponential: exp(tau A) b by Krylov projection (src/Expm/ExpmLib.fypp) -------------------------------
 * expm(A) of stdlib_linalg, which ExpmLib.fypp:12, 207 applies to the small projected matrix: E = exp(A) for an n x n column-major
 * matrix of `dtype` (LK_F64 / LK_C128; lda, lde in elements; E may be A).  HOST ONLY -- no context, no device, no LAPACK: scaling
 * and squaring with the [13/13] Pade approximant (Higham 2005) and an LU factorisation with partial pivoting (csrc/lk_expm.h).
 * n = 0 is LK_OK; n < 0, a null pointer or a leading dimension below n is LK_ERR_INVALID. */
int lk_expm_dense(int dtype, int n, const double *A, int64_t lda, double *E, int64_t lde);
/* kexpm(c, A, b, tau, tol, info, trans, kdim), vector form: src/Expm/ExpmLib.fypp:128-232 (krylov_exptA, :365-392, is this call
 * with tol = atol_dp and kdim = 30).  c = column jc of Bc (overwritten) ~ exp(tau op(A)) b, b = column jb of Bb (read only).
 * X: workspace of the CALLER, >= kdim + 1 columns of the same context, dtype and n_local -- the call allocates no device memory (a
 * time stepper makes it thousands of times); on return it holds the Krylov basis.  1 <= kdim <= min(ncols(X) - 1, 512).
 * Same `info` and same c as the reference, on another schedule: ||b||^2 stays on the device, where one kernel forms X(:, 1) = b / ||b||
 * out of place (:186-187 take three passes and a host round trip); the Arnoldi steps (:196, tolerance atol_dp) are enqueued back to back as
 * in lk_arnoldi_segments and delivered one by one; for each the host evaluates E = expm(tau H(:kp, :kp)), kp = k + 1, and
 * err_est = |E(kp, 1) beta| (:207, :215) while the device runs ahead -- at most 24 steps, which touch only columns of X the result
 * does not use -- and stops the factorisation at the first step with err_est <= tol (:218); an Arnoldi breakdown at step k gives
 * kp = k and err_est = 0 (:200-204, :215).  The projection c = X(:, :kp) (beta E(:kp, 1)) then runs ONCE (:210-211 repeat it after
 * every step: O(k^2) column passes of which the last survives).  One host synchronisation beyond those of the factorisation.
 * info = kp when err_est <= tol (after a breakdown too); kp = 1 and c = 0 for b = 0 (:180-184); -1 when kdim steps did not reach
 * tol -- c is then the kdim-step approximation (:223-231).  err_est may be NULL.
 * LK_ERR_INVALID, with nothing written: kdim out of range; c a column of X, or the same column as b; b one of the columns
 * [0, kdim] of X; operator and vectors of different shape, kind or context; a ROW-SHARDED context (nranks > 1).
 * Not provided: row-sharded contexts, and the Newton-Krylov layer built on the propagator. */
int lk_kexpm(lk_linop_t A, int trans, lk_basis_t Bb, int jb, lk_basis_t Bc, int jc, lk_basis_t X, double tau, double tol, int kdim,
             int *info, double *err_est);

/* ---- qr_with_pivoting and the block form of kexpm ------------------------------------------------------------------
 * Largest singular value of an m x n column-major matrix of `dtype` (lda in elements): `norm(., 2)` of stdlib_linalg, which
 * ExpmLib.fypp:346 applies to the small p x p block of kexpm_mat's error estimate.  HOST ONLY, like the dense exponential above -- no
 * context, no device, no LAPACK: one-sided Jacobi (Hestenes) rotations on a packed copy (csrc/lk_expm.h).  m or n = 0 gives
 * out = 0 and LK_OK; a negative size, a null pointer or lda < m is LK_ERR_INVALID. */
int lk_norm2_dense(int dtype, int m, int n, const double *A, int64_t lda, double *out);
/* qr_with_pivoting(Q, R, perm, info, tol): src/Krylov/qr.fypp:32-107 (swap_columns :176-202), on columns [j0, j0 + p) of a panel,
 * p <= 512.  R: host p x p column-major (leading dimension ldr elements) of the basis dtype, zeroed by the call (:42; rows p..ldr-1
 * are not touched); perm: p ints, 1-BASED like the reference's (:49): on return column i of Q R is column perm(i) of the input.
 * Rii(i) = Q(i)%dot(Q(i)) (:50) comes from multi-column dot passes, four columns each.  Column j: the first maximum of |Rii| (:54; a
 * NaN counts as the largest, so a column that holds one is taken at once and ends the call at the norm test) below
 * tol => columns j..p are re-drawn from the counter generator (stream 0x5EED + panel column + 1, as the re-draw of the unpivoted
 * factorisation above), each orthogonalised against the columns before it and normalised, info = j, and the loop exits (:55-66).
 * Otherwise columns j and idx are exchanged IN PLACE on the device (one kernel, two reads and two writes per element, no temporary;
 * :192-194 are three copies through a fresh vector) together with R(:min(j, idx) - 1, .), Rii and perm (:196-201); beta = ||q_j||
 * (:71), NaN => LK_ERR_NAN "|beta| = NaN detected! Abort" (:73-77); |beta| < tol => info = j, R(j, j) = 0, re-draw, Gram-Schmidt, new
 * norm (:79-85; the reference hands `info` to that Gram-Schmidt step, which clears it again: here it stays j), else R(j, j) = beta;
 * q_j scaled (:90).  The trailing update (:93-97) is ONE classical pass, as there, but over all remaining columns at once:
 * h = q_j^H Q(:, j+1:p) by the multi-column dot kernel and Q(:, j+1:p) -= q_j h by the tall-skinny product, four columns per launch
 * pair, one host synchronisation per column j; R(j, i) = h_i.  Rii(i) -= R(j, i)**2 (:100-103) on the host -- for the complex kind
 * Rii is complex and that is the complex SQUARE, not |R(j, i)|^2, as in the reference.
 * Host-synchronous.  No device memory is allocated beyond the context's grow-once workspaces.
 * LK_ERR_INVALID, with nothing written: a null argument, a bad column range, p > 512, ldr < p, and a ROW-SHARDED context (nranks > 1:
 * the re-draw and the reductions of this schedule have not been walked through for a row partition). */
int lk_qr_pivot(lk_basis_t Q, int j0, int p, double *R, int64_t ldr, int *perm, double tol, int *info);
/* kexpm(C, A, B, tau, tol, info, trans, kdim), block form (kexpm_mat): src/Expm/ExpmLib.fypp:234-363.  C = columns [jc0, jc0 + p) of Bc
 * (overwritten) ~ exp(tau op(A)) B, B = columns [jb0, jb0 + p) of Bb (read only).  nk: the largest number of BLOCK Arnoldi steps (the
 * reference sets nk = kdim * p, :276; the mirrors compute it).  X: workspace of the CALLER with at least p (nk + 1) <= 512 columns of
 * the same context, dtype and n_local; on return it holds the block Krylov basis.  No device memory is allocated beyond the context's
 * grow-once workspaces.
 * Start: X(:, :p) = B, pivoting qr with tolerance atol_dp (its info is discarded, :297), R := permcols(R, invperm(perm)); ||R||_F = 0
 * gives C = 0, kpp = p and err_est = 0 (:299-302); else the unpivoted qr of the orthonormal block that initialize_krylov_subspace
 * runs (:304, src/Krylov/utilities.fypp:44-46).  Step k = 1..nk (:306-351): ONE block Arnoldi step (kstart = kend = k, tolerance
 * atol_dp, :314), kp = k p; info = kp there => kpp = kp (:317-321), else kpp = kp + p; E = expm(tau H(:kpp, :kpp)) (:324);
 * err_est = 0 after a breakdown, else the spectral norm of E(kp+1:kpp, :p) R (:342-347); stop at err_est <= tol (:349).  One host
 * synchronisation per step (no look-ahead as in the vector form above).  The projection C = X(:, :kpp) (E(:kpp, :p) R) runs ONCE behind the loop,
 * the small product on the host (:327-339 repeat it after every step and keep the last).
 * info = kpp when err_est <= tol, else -1 -- C is then the nk-step approximation (:354-362).  err_est may be NULL.
 * LK_ERR_INVALID, with nothing written: p < 1; nk < 1 or p (nk + 1) beyond the workspace or 512; a column of C inside X or shared with
 * B; a column of B among the columns [0, p (nk + 1)) of X; operator and panels of different shape, kind or context; a ROW-SHARDED
 * context (nranks > 1). */
int lk_kexpm_block(lk_linop_t A, int trans, lk_basis_t Bb, int jb0, lk_basis_t Bc, int jc0, int p, lk_basis_t X, double tau, double tol,
                   int nk, int *info, double *err_est);

/* ---- restarted GMRES(kdim) as one call ----------------------------------------------------------------------------------
 * gmres(A, b, x, info, rtol, atol, preconditioner, options, transpose, meta): src/IterativeSolvers/GMRES/gmres.fypp:65-255.
 * Solves op(A) x = b; x = column jx of Bx is the initial guess and is overwritten, b = column jb of Bb is read only.  M: NULL, or a
 * RIGHT preconditioner given as an engine operator, always applied as LK_OP_N: the step is V(k+1) = op(A) M V(k) (:155-165) -- one
 * Arnoldi batch on the product of the two operators, see lk_linop_compose_create -- and the update x += M (V y) (:201-202).  The
 * reference hands k, beta and tol to the preconditioner's apply; a fixed operator has no use for them.  (The flexible variant,
 * fgmres.fypp, with a fixed operator IS this call; a preconditioner that varies needs a host callback per step and is not provided.)
 * V: workspace of the CALLER, as in lk_kexpm: >= kdim + 1 columns, >= kdim + 2 with M (the extra column is the scratch vector of the
 * product operator, which lives on the call's stack); 2 <= kdim <= 512.  No device memory is allocated beyond the context's grow-once
 * workspaces.  options%kdim and %maxiter are the arguments of those names: at most maxiter + 1 cycles (:131).
 * Schedule.  ONE host synchronisation at entry (||b|| for tol = atol + rtol ||b||, :106, and ||x|| for the test at :134), then ONE PER
 * CYCLE plus those of the Arnoldi batch's deliveries.  A cycle starts with lk_linop_residual into V(:, 0), the sum left on the device,
 * where the normalisation reads it (:134-143); beta reaches the host with the first delivery of the batch.  The inner steps are one
 * Arnoldi batch with tolerance tol, delivered step by step as in lk_arnoldi_segments: the host applies the Givens rotations and appends
 * |e(k+1)| to the history while the device runs ahead, and stops the batch at |e(k+1)| < tol (:178-195; the steps run ahead touch only
 * columns the update does not read).  A batch that ends on H(k+1, k) <= tol with the residual still >= tol is followed by the remaining
 * steps one by one, the new vector left unscaled, as the reference does (:171-172; lk_arnoldi has normalised the vector of the step it
 * stopped at, which is undone to rounding; a vector below atol_dp it has REPLACED by a normalised random one, qr.fypp:146-162, and
 * the call goes on with that one where the reference keeps the tiny vector -- reachable only with tol < atol_dp = 1e-15).  The triangular solve (:199-200) is back
 * substitution on the host -- a zero pivot is LK_ERR_INVALID "TRTRS failed" --, dx = V(:, :k) y goes to V(:, kdim), M dx to V(:, 0),
 * x += dx.  The cycle ends with lk_linop_residual into V(:, 0) and its norm (:205-214); when the solve goes on, the NEXT cycle
 * normalises THIS vector instead of forming it again (:134-142 compute the same vector the same way): the call applies ONE PRODUCT
 * FEWER PER RESTART than the reference's loop counts, and three passes fewer.
 * A START RESIDUAL OF EXACTLY ZERO (x the exact solution already -- a warm start from a converged step --, or b = 0 with x = 0): the
 * reference divides by beta = 0 (gmres.fypp:142-143) and returns NaN.  Here the call returns LK_OK with x unchanged, info = 0,
 * n_inner = n_outer = 0, nres = 1 and res[0] = 0, for both kinds, with or without M, whatever atol is; columns of V the call may write
 * are written.  beta reaches the host with the first delivery anyway: the case costs no synchronisation on any other path.  A residual
 * below tol that is not zero takes one step, as in the reference.  This covers the residual the call STARTS from.  With tol = 0 (rtol = atol = 0,
 * or b = 0 with atol = 0 and x != 0) no residual counts as converged, a zero one included: a later cycle that starts from a residual of
 * exactly zero ends in LK_ERR_INVALID "TRTRS failed" (real kind, a zero pivot) or LK_ERR_NAN (complex kind, the rotation divides by it).
 * info = +n_iter when converged, -n_iter otherwise (:234-238); n_iter counts the inner steps plus one per cycle.  res (may be NULL)
 * receives at most res_cap entries of the residual history, nres its full length, at most 1 + (maxiter + 1)(kdim + 1); n_inner and
 * n_outer as in gmres_dp_metadata (IterativeSolvers.fypp:153-170).  nres, n_inner and n_outer may be NULL.
 * LK_ERR_INVALID, with nothing written: a null A, V or info; kdim out of range; the workspace too narrow; x or b one of the columns of
 * V the call writes ([0, kdim], [0, kdim + 1] with M); x and b the same column; operator, preconditioner and vectors of different
 * shape, kind or context; a ROW-SHARDED context (nranks > 1).  LK_ERR_NAN: ||b|| or a residual norm is not finite. */
int lk_gmres(lk_linop_t A, int trans, lk_linop_t M, lk_basis_t Bb, int jb, lk_basis_t Bx, int jx, lk_basis_t V, double rtol, double atol,
             int kdim, int maxiter, double *res, int64_t res_cap, int64_t *nres, int *n_inner, int *n_outer, int *info);

/* ---- conjugate gradient as one call --------------------------------------------------------------------------------------
 * cg(A, b, x, info, rtol, atol, preconditioner, options, meta): src/IterativeSolvers/CG/CG.fypp:60-196.
 * Solves A x = b for a symmetric / Hermitian positive definite A, applied as LK_OP_N only (cg has no transpose argument); x = column jx
 * of Bx is the initial guess and is overwritten, b = column jb of Bb is read only.  M: NULL, or a FIXED preconditioner given as an
 * engine operator, z = M r (:113, :134).  W: workspace of the CALLER, as in lk_gmres and lk_kexpm: >= 3 columns (r, p, Ap in columns
 * 0, 1, 2), >= 4 with M (z in column 3), same context, kind and n_local.  No device memory is allocated beyond the context's grow-once
 * workspaces (the iteration's scalars and the history ring are one of them).  options%maxiter is the argument of that name.
 * What it computes.  tol = atol + rtol ||b|| (:87).  r = b - A x, the product only when ||x|| > 0 (:108-109); z = M r, p = z,
 * rho = r.z, or p = r, rho = r.r (:113-116); res[0] = sqrt|rho| (:119).  Iteration i = 1..maxiter (:123): Ap = A p (:125);
 * alpha = rho / (p.Ap) (:127); x += alpha p (:129); r -= alpha Ap (:131); z = M r and rho' = r.z, or rho' = r.r (:134-137); the residual
 * sqrt|rho'| -- rho is complex for the complex kind (:141-145) -- joins the history (:148-149); residual < tol ends the loop converged,
 * BEFORE the direction update (:151-154); else beta = rho' / rho (:157), p = (z or r) + beta p (:160-164), rho <- rho' (:167).
 * info = +n_iter when converged, -n_iter otherwise (:175-179); maxiter = 0 gives nres = 1, info = 0.  A start residual below tol that
 * is not zero still takes one iteration, as there.  res (may be NULL) receives at most res_cap entries of the history, nres (may be
 * NULL) its full length, at most maxiter + 1.
 * Schedule.  ONE host synchronisation at entry (||b|| and ||x||), then one PER DELIVERY and none per iteration.  The start residual is
 * lk_linop_residual's, its sum left on the device (x = 0: a copy of b and its dot).  Per iteration, on the context's stream: the
 * operator's kernels; p.Ap by the dot kernel and the engine's fixed-order reduce step; ONE launch that forms alpha on the device and
 * updates x and r in one pass (four reads, two writes; the reference's two axpbys and the norm read take seven), leaving the per-block
 * sums of r.r; with M the operator's kernels for z and the dot kernel for r.z; ONE one-block launch that finishes rho' in fixed order,
 * writes it to the iteration's history slot, forms beta, raises the device stop flag at sqrt|rho'| < tol and rotates rho; ONE launch
 * for p = z + beta p, beta read on the device.  The three are passes that run inside k_axpby's symbol, which adds no kernel instance.
 * No floating-point atomics, nothing persistent, nothing that waits inside a launch.
 * Complex quotients are (a + ib) / (c + id) = ((a + b t) / s, (b - a t) / s), t = d / c, s = c + d t for |c| >= |d|, and
 * ((a t + b) / s, (b t - a) / s), t = c / d, s = c t + d otherwise, written out in the kernel.
 * The host enqueues iterations at most 24 ahead of the last one whose history entry it has read (the look-ahead of
 * lk_arnoldi_segments); history slots and the stop flag come back through pinned memory behind an event every 8 iterations and behind
 * the last.  Every kernel of the batch carries the batch's guard; the direction update carries the number of the iteration it OPENS,
 * so after a stop in iteration i nothing of iteration i + 1 runs: x is exactly the reference's x at exit, and columns 0 and 1 of W
 * hold the r and p the reference leaves the loop with.  The launches enqueued past a stop are no-ops: at most 24 iterations' worth.
 * Defined where the reference is not.  A START RESIDUAL OF EXACTLY ZERO (x the exact solution already, or b = 0 with x = 0): the
 * reference computes 0 / 0 at :127 and returns NaN.  Here the call returns LK_OK with x unchanged, info = 0, nres = 1 and res[0] = 0,
 * as lk_gmres does; the columns of W may be written.  A rho or p.Ap that is not finite, or p.Ap = 0 (A not definite): LK_ERR_NAN; the
 * iteration that meets such a p.Ap writes nothing.  ||b|| or ||x|| not finite: LK_ERR_NAN before anything is written.
 * LK_ERR_INVALID, with nothing written: a null A, W or info; maxiter < 0; the workspace too narrow; x or b overlapping one of the
 * columns of W the call writes ([0, 3), [0, 4) with M); x and b overlapping; operator, preconditioner and vectors of different shape,
 * kind or context; a ROW-SHARDED context (nranks > 1).
 * Not provided: row-sharded contexts; a preconditioner that varies per iteration (it needs a host callback per iteration); the product
 * fused into the update for row-local operators (what "fuse_rowop" does for the Arnoldi sweeps). */
int lk_cg(lk_linop_t A, lk_linop_t M, lk_basis_t Bb, int jb, lk_basis_t Bx, int jx, lk_basis_t W, double rtol, double atol, int maxiter,
          double *res, int64_t res_cap, int64_t *nres, int *info);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTKRYLOV_HIP_H */
