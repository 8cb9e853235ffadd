/*
 * omp_amg_amd.h -- device-resident entry points of libomp_amg_amd.so.
 *
 * The drop-in host ABI (amg_setup.h) copies COO in and the hierarchy out over
 * PCIe.  Callers that already hold the matrix in HBM (the bench, a GPU solver)
 * use these: COO already on the device in, hierarchy kept in HBM, optional
 * export into a host `struct amg_setup_data`.
 *
 * Reference interface replaced: amg_setup() (amg_setup.h:5), split at the
 * host/device boundary.
 */
#ifndef OMP_AMG_AMD_H
#define OMP_AMG_AMD_H

#include <stddef.h>
#include <stdint.h>
#include "amg_setup.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amgd_hier amgd_hier;

/* per-phase device times (ms) and work counters of the last setup */
typedef struct {
  double t_total_ms, t_build_ms, t_coarsen_ms, t_smoother_ms, t_interp_ms, t_rap_ms, t_copy_ms;
  double rap_kernel_ms;          /* fused/ordered SpGEMM kernels inside RAP, event-timed */
  uint64_t rap_out_nnz;          /* sum over levels of nnz(A_{l+1}) */
  uint64_t rap_bytes;            /* algorithmic HBM bytes of the RAP SpGEMMs */
  uint64_t rows0, nnz0;
  uint32_t nlevels, ub_events;   /* ub_events: inputs outside the reference's defined domain */
  size_t peak_bytes;
  double spmv_kernel_ms;         /* whole-matrix long-row SpMV kernels (k_spmv_pipe), event-timed */
  uint64_t spmv_bytes;           /* their bytes with x gathered once per entry */
  uint64_t spmv_bytes_strict;    /* their algorithmic HBM bytes: x read once per product */
  uint64_t spmv_launches, rap_launches;   /* kernel launches behind spmv_/rap_kernel_ms */
  /* the long-row SpMV per shape: RW = 4 / 16 / 64 rows per wavefront (k_spmv_pipe<.., RW>) */
  double spmv_rw_ms[3];
  uint64_t spmv_rw_bytes_strict[3], spmv_rw_launches[3];
  /* the first AMGD_UB_LOG reference-undefined events: site (1 find_support theta -> 0, 2 one-row R,
     3 a sweep removed nothing, 4 selections past nnz(R) + nc, 5 skeleton stalled) and level */
  uint8_t ub_site[8], ub_level[8];
} amgd_stats;
#define AMGD_UB_LOG 8

int amgd_init(int device);                       /* 0 = ok; <0 = no usable HIP device */
/* release every device buffer, event and the stream of the library (hierarchies
   not yet freed become invalid); amgd_init may be called again afterwards */
void amgd_shutdown(void);
/* Global dot products (PCG, Lanczos): 1 = summed in the reference's left-to-right
   order (default; hierarchy bit-identical to the reference), 0 = fixed-order tree
   (faster; differs in the last bits, which the reference's chaotic constraint
   solve can amplify -- DESIGN.md "Parity").  Env AMGD_FAST_DOTS=1 sets 0. */
void amgd_set_exact_dots(int on);
const char *amgd_error(void);
/* device pointers in, hierarchy out (kept in HBM).  flags: bit0 = also keep host copies */
int amgd_setup_device(uint64_t nz, const uint32_t *dAi, const uint32_t *dAj, const double *dAv,
                      amgd_hier **out, int flags);
int amgd_hier_export(const amgd_hier *h, struct amg_setup_data *data);  /* D2H into the ABI struct */
void amgd_hier_free(amgd_hier **h);
void amgd_get_stats(amgd_stats *st);
/* One AMG V-cycle on the kept hierarchy (the reference's amg_exec, amg.c:114-169; DESIGN.md
   "Solve"): dx = cycle(db), device vectors of n0 doubles in level-0 row order (row =
   global id - 1); db is not modified.  flags bit 0: subtract the mean of x (a singular
   operator, crs_setup's null_space).  The solve plan (level-ordered layout, W', work
   vectors) is built on the first call and freed with the hierarchy.  Runs on the library
   stream; amgd_dev_sync waits for it.  0 ok; -1 bad or empty hierarchy; -2 out of HBM
   (reason in amgd_error(), everything the failed call allocated released -- the plan, or
   the mean removal's reduction, after which dx is not written); -3 a partitioned hierarchy
   without flag bit 2 (below).
   AMGD_VC_FUSED=0: only the setup's own kernels (the composed path, same bits);
   AMGD_VC_TAIL=0: no one-workgroup coarse tail (same bits).
   A partitioned hierarchy is solved with flag bit 2 (value 4) set: the call is then
   collective (every rank makes it, on the library communicator of the setup) and works on the
   rank's own rows, which a caller written for one GPU would not expect -- so without the bit
   the call returns -3 and touches nothing.  dx and
   db are still whole-length level-0 vectors, but the call reads only this rank's rows of db
   (amgd_hier_rows) and writes only this rank's rows of dx, bit-identical to the one-GPU
   cycle on the gathered hierarchy.  flags bit 1 (value 2) completes dx on every rank with one
   allgatherv.  Bit 0 needs the sequential sum over the whole level-ordered x: x is completed
   on every rank first (one more allgatherv of 8 B per position of the distributed levels),
   then every rank takes the same sum.  Out of HBM while planning follows the partitioned
   setup's rule: with the collective guard every rank returns -2 and releases everything,
   without it a multi-process job aborts with the reason.
   AMGD_VC_HALO=0: the exchanges complete whole F segments (allgatherv) instead of moving the
   referenced entries only (same bits); AMGD_VC_REPL_ROWS=n: the levels whose slice of the
   level-ordered vector has at most n positions run replicated on every rank (same bits). */
int amgd_solve_device(amgd_hier *h, double *dx, const double *db, int flags);
/* this rank's level-0 row range [*r0, *r1) of the hierarchy; one GPU: [0, n0).  0 ok, -1 bad
   hierarchy or another communicator than the setup's */
int amgd_hier_rows(const amgd_hier *h, uint32_t *r0, uint32_t *r1);
/* the last solve's collectives and the bytes all ranks together sent in them (the same numbers
   on every rank: counted from the plan's lists, not measured); one GPU: 0, 0 */
void amgd_solve_comm_stats(uint64_t *collectives, uint64_t *bytes_sent);
/* cycles run so far, their device-event time, and the algorithmic HBM bytes of one cycle of
   the hierarchy solved last (12 B per matrix entry per pass, 8 B per vector element read or
   written, from shapes) */
void amgd_solve_stats(uint64_t *cycles, double *ms, uint64_t *bytes);
/* One V-cycle on each of nrhs right-hand sides in one call (DESIGN.md "Solve", "Several
   right-hand sides").  dB and dX are column-major device blocks: column j starts at + j*ld,
   ld >= n0.  Column j of dX receives bit for bit what
   amgd_solve_device(h, dX + j*ld, dB + j*ld, flags) writes, for every nrhs >= 1 and both
   values of flag bit 0 (the mean is removed per column, each column's sum taken left to right
   in the level-ordered layout through the exact-dot path).  dB is not modified; entries
   [n0, ld) of every column of dX are not written.  The columns run in groups of 8, 4 or 2
   (greedily; the sizes allowed by default are the measured ones of DESIGN.md), each group one
   pass over the hierarchy's matrices with the group's vectors interleaved; a column left over
   takes the single-vector cycle, and a level whose matrix has a row of more than 4 096
   entries runs its part of the cycle column by column through the single-vector kernels.
   AMGD_VC_MRHS_K=8,4,2 lists the allowed group sizes (0: none).  AMGD_VC_MRHS_FAMILY=1 / 2
   forces the short-row / the long-row kernels on every row shape (default: by the matrix's
   mean row length; same bits either way).  Route counters (amgd_route_stats): vc_mr_thr and
   vc_mr_wave count the K-column products by kernel family, vc_mr_single the columns sent
   through the single-vector cycle, vc_mr_comp the per-column passes of a level that fell
   back because of an outlier row.
   The interleaved work vectors (4 N K doubles for the largest group size K used so far) are
   kept with the solve plan.
   0 ok; -1 nrhs < 1, ld < n0, a null pointer or an empty hierarchy; -3 a partitioned
   hierarchy, with or without flag bit 2: the multi-rank form of this call does not exist (solve
   the columns one by one with amgd_solve_device and flag bit 2); -2 out of HBM: everything
   the call allocated is released, the hierarchy and its single-vector plan stay usable. */
int amgd_solve_device_n(amgd_hier *h, double *dX, const double *dB, int nrhs, uint64_t ld, int flags);
/* amgd_solve_device_n calls and columns so far, the calls' device-event time (a timer of
   their own: amgd_solve_stats does not see these calls, except for the columns that took the
   single-vector cycle), and the algorithmic bytes of the last call: 12 B per matrix entry
   per pass ONCE per group (the matrices of a level that fell back column by column: once per
   column), 8 B per vector element read or written times the group's columns; the fallback's
   copies between the interleaved and the contiguous vectors are not counted */
void amgd_solve_n_stats(uint64_t *calls, uint64_t *columns, double *ms, uint64_t *bytes);
/* the hierarchy crs_setup (crs.h) keeps in HBM, copied into the ABI struct -- the same
   layout amg_setup fills; free with free_data */
struct crs_data;
int amgd_crs_export(const struct crs_data *crs, struct amg_setup_data *data);
/* crs_solve (crs.h) on nrhs right-hand sides: X and B are column-major host blocks of the
   local dofs (column j at + j*ld, ld >= the n of crs_setup).  Column j of X receives what
   crs_solve(X + j*ld, data, B + j*ld) writes: b of the dofs sharing an id summed in ascending
   local index, x written back to every dof of the id, id-0 dofs untouched; B is not modified.
   One amgd_solve_device_n call on the assembled system.  0 ok; -1 bad arguments; -2 out of
   HBM; -3 comm->np > 1 (as amgd_solve_device_n on a partitioned hierarchy) */
int amgd_crs_solve_n(double *X, struct crs_data *data, const double *B, int nrhs, uint64_t ld);
/* ---- A x = b on the kept hierarchy: restarted flexible GMRES, the V-cycle as the right
   preconditioner (DESIGN.md "Krylov").  GMRES and not CG: the cycle is not a symmetric
   operator.  Classical Gram-Schmidt applied twice; the residual estimate of the recurrence
   decides when a restart ends, the recomputed true residual ||b - A x|| when the solve does. */
#define AMGD_KRYLOV_MAX_RESTART 64
typedef struct {
  double rtol, atol;     /* converged when ||b - A x|| <= max(rtol*||b||, atol) */
  uint32_t restart;      /* basis size m, 1..AMGD_KRYLOV_MAX_RESTART; 0: 30 */
  uint32_t maxit;        /* cap on inner iterations over all restarts; 0: 100 */
  uint32_t flags;        /* bit 0: ordered dots (below); bit 1: dx holds the initial guess; bit 2
                            (value 4): the collective call on a row-partitioned hierarchy; bit 3
                            (value 8): that call completes dx on every rank (below) */
} amgd_krylov_opts;
typedef struct {
  uint32_t its, restarts, cycles, converged;
  double bnorm, r0, resid;   /* ||b||, the first residual norm, the last TRUE residual norm */
} amgd_krylov_info;
/* dx and db: device vectors of n0 doubles in level-0 row order, as for amgd_solve_device; db is
   not modified.  hist (host, may be NULL): entry k receives the residual estimate after inner
   iteration k + 1, for the first hist_cap iterations.  A hierarchy with a null space has the
   cycle applied with its flag bit 0, as crs_solve does.
   flags bit 0, ordered: every dot is the left-to-right sum from +0 of the rounded products
   (amgd_dot with the exact summation forced on for the call, the global setting restored
   afterwards) -- the verification path, which a host restatement reproduces bit for bit.
   Default, fused: all dots of a Gram-Schmidt pass in one sweep over the basis, partial sums
   added in a fixed order (two runs give the same bits), one host synchronisation per inner
   iteration.  Both paths share the update, scale and combine kernels.
   The workspace (2 m + 4 vectors) is kept with the hierarchy's solve plan, regrown when m
   grows, and freed by amgd_hier_free.
   0 converged; 1 maxit reached (dx holds the last iterate, info is filled); -1 a null h, dx,
   db, o or info, an empty hierarchy, restart > AMGD_KRYLOV_MAX_RESTART, a negative or NaN rtol
   or atol (nothing is touched); -2 out of HBM (reason in amgd_error(), everything the call
   allocated released, the hierarchy and its solve plan stay usable, dx not written); -3 a
   partitioned hierarchy called without flag bit 2 (nothing allocated); -4 a non-finite norm
   appeared (dx not written).  Route counters: kry_it inner iterations, kry_mdot fused multi-dot
   launches, kry_odot ordered dots.
   A row-partitioned hierarchy (DESIGN.md "Krylov on the row-partitioned hierarchy") is solved
   with flag bit 2, the value of amgd_solve_device's: the call is collective, db and dx are
   whole-length level-0 vectors of which only this rank's rows (amgd_hier_rows) are read (dx: with
   flag bit 1) and written; flag bit 3 completes dx on every rank with one allgatherv at the
   end.  On a one-GPU hierarchy both bits change nothing.  V, Z, w, x and r hold the rank's own
   rows (2 m + 4 vectors of that length) beside one whole-length operand of the level-0 product,
   whose halo entries are fetched per product (AMGD_VC_HALO=0: one allgatherv of the segments);
   the ordered path adds two whole-length vectors when it first runs.  Ordered: every operand of
   a dot is completed on every rank and the dot taken redundantly, so x on the own rows, info
   and hist are bit for bit the one-GPU ordered solve on the gathered hierarchy, whatever the
   ranks, the split and the cycle's mode.  Fused: every rank's multi-dot on its own rows, the
   ranks' sums gathered by one allgatherv and added in rank order by one kernel -- bit for bit
   the one-GPU fused solve on one rank, deterministic for a given rank count and split, and
   identical on every rank, so return code, info and hist are the same everywhere.  Route
   counters: kry_p_xch exchanges before a level-0 product, kry_p_comb rank-order combines. */
int amgd_krylov_device(amgd_hier *h, double *dx, const double *db, const amgd_krylov_opts *o,
                       amgd_krylov_info *info, double *hist, uint32_t hist_cap);
/* amgd_krylov_device calls and inner iterations so far, the calls' device-event time (a timer
   of their own) */
void amgd_krylov_stats(uint64_t *calls, uint64_t *its, double *ms);
/* collectives entered and bytes all ranks sent in the last amgd_krylov_device call, counted from
   the plan like amgd_solve_comm_stats, the cycles' included; the same on every rank.  A fused
   call with its > 0, cyc one cycle's collectives, px 1 when a level-0 product has an exchange
   and g 1 with a guess makes
     1 + g (px + 1) + its (cyc + px + 3) + (restarts + 1) (px + 1) + (bit 3 ? 1 : 0);
   one rank: 0 */
void amgd_krylov_comm_stats(uint64_t *collectives, uint64_t *bytes);
/* amgd_krylov_device in crs_solve's id handling (crs.h): b of the local dofs sharing an id
   summed in ascending local index, x written to every dof of the id, id-0 dofs untouched, b
   not modified; with flag bit 1 the guess of an id is x at its first local dof.  Returns what
   amgd_krylov_device returns (x is written for 0 and 1 only).  comm->np > 1 (collective): b is
   assembled as crs_solve assembles it, the guess of an id is x at the first local dof of the
   lowest rank that carries the id; a partitioned hierarchy is solved with flag bits 2 and 3, the
   replicated setup mode completes b on every rank and runs the one-GPU solver on each */
int amgd_crs_krylov(double *x, struct crs_data *data, const double *b,
                    const amgd_krylov_opts *o, amgd_krylov_info *info);
/* ---- A X = B for nrhs right-hand sides of one operator: nrhs independent flexible GMRES solves
   run in lock-step (DESIGN.md "Krylov on several right-hand sides").  dB and dX are column-major
   device blocks, column j at + j*ld, ld >= n0, as for amgd_solve_device_n; info has nrhs
   entries, rcs (may be NULL) nrhs, and column j's history goes to hist + j*hist_cap (hist may
   be NULL).  Column j of dX, info[j], rcs[j] and column j's history are bit for bit what
   amgd_krylov_device(h, dX + j*ld, dB + j*ld, o, &info[j], hist + j*hist_cap, hist_cap) writes
   and returns, on both dot paths, for every nrhs >= 1, every slot count and every allowed group
   size: a column's result does not depend on which other columns ran beside it.  dB is not
   modified, rows [n0, ld) of dX are not written, flag bit 1 reads column j of dX as column j's
   guess.
   Up to 8 columns are in flight at a time, each in a slot of 2 m + 4 vectors (AMGD_KRY_SLOTS
   lowers the count; the default is DESIGN.md's measured one); a finished column's slot goes to
   the next pending column at the next step.  Per step the cycles of the active columns run
   through the K-column cycle and their level-0 products through a K-column product, in groups
   of 8 / 4 / 2 under the AMGD_VC_MRHS_K mask, so the matrices are streamed once per group; the
   Gram-Schmidt passes of all active columns are single launches with one host wait per step
   (fused path; the ordered path keeps its per-column ordered dots).  AMGD_KRY_MRHS_FAMILY=1 / 2
   forces the short-row / long-row product kernel (default: by mean row length, long from 16).
   The slots' workspace, S (2 m + 4) n0 8 bytes (68.7 GB at m = 30, S = 8, n0 = 256^3), is kept
   with the hierarchy, regrown when S or m grows and freed by amgd_hier_free.
   rcs[j]: 0, 1 or -4 as amgd_krylov_device returns them; with -4 column j of dX is not written
   and the other columns go on.  Returns 0 if every column is 0, else -4 if any column is -4,
   else 1.  -1 a bad argument (a null h, dX, dB, o or info, nrhs < 1, ld < n0, an empty
   hierarchy, or amgd_krylov_device's option checks): nothing is touched.  -3 a partitioned
   hierarchy.  -2 out of HBM: while planning or allocating the workspace, nothing is written;
   during the iteration, the columns already finished keep their result and rcs, the others get
   rcs[j] = -2 and are not written; either way everything the call allocated is released and the
   hierarchy, its solve plan and the single solver's workspace stay usable.
   Route counters: kry_n_step lock-step steps, kry_n_mixed steps whose active columns stood at
   two or more different j, kry_n_prod K-column product launches, kry_n_single columns sent
   through the single-vector cycle or product as a group's leftover, kry_n_comp per-column
   products of a matrix with a row of more than 4 096 entries. */
int amgd_krylov_device_n(amgd_hier *h, double *dX, const double *dB, int nrhs, uint64_t ld,
                         const amgd_krylov_opts *o, amgd_krylov_info *info /* nrhs */,
                         int *rcs /* nrhs, may be NULL */, double *hist /* may be NULL */, uint32_t hist_cap);
/* amgd_krylov_device_n calls, columns and lock-step steps so far, the calls' device-event time
   (a timer of their own) */
void amgd_krylov_n_stats(uint64_t *calls, uint64_t *columns, uint64_t *steps, double *ms);
/* amgd_crs_krylov on nrhs columns: X and B are column-major host blocks of the local dofs
   (column j at + j*ld, ld >= the n of crs_setup), as amgd_crs_solve_n is to crs_solve; column j
   of X, info[j] and rcs[j] (may be NULL) are what amgd_crs_krylov gives on that column.  One
   amgd_krylov_device_n call; returns what it returns, -3 with comm->np > 1 */
int amgd_crs_krylov_n(double *X, struct crs_data *data, const double *B, int nrhs, uint64_t ld,
                      const amgd_krylov_opts *o, amgd_krylov_info *info, int *rcs);
/* ---- multi-GPU: row-sharded setup over the GPUs of one node (DESIGN.md "Multi-GPU") ----
   Every rank calls amgd_setup_device on the same matrix; the row-independent heavy
   kernels (SpGEMMs, Q factors) are split by work across the ranks and completed by
   an in-place allgatherv, so every rank ends with the same, bit-identical hierarchy.
   No reference interface corresponds: the reference's setup is serial
   (amg_setup.c:60); crs_setup's comm (crs.h:15) is where a caller passes its ranks. */
int amgd_comm_rccl_uid(unsigned char uid[128]);     /* rank 0: fresh RCCL unique id */
int amgd_comm_init_rccl(int rank, int size, const unsigned char uid[128]);
/* host transport: bufs[b] is a device buffer whose range s holds bytes
   [offs[b*(size+1)+s], offs[b*(size+1)+s+1]); rank `rank` fills its range, the callback
   must leave every range filled on every rank.  Returns 0 on success. */
typedef int (*amgd_allgatherv_fn)(void *user, int nbuf, void *const *bufs, const uint64_t *offs,
                                  int rank, int size);
int amgd_comm_init_host(int rank, int size, amgd_allgatherv_fn fn, void *user);
int amgd_comm_init_sim(int nshards);   /* one process computes all shards in turn (tests) */
void amgd_comm_free(void);             /* back to one GPU */
int amgd_comm_size(void);
int amgd_comm_rank(void);
/* Partitioned mode (the north_star layout): with a multi-process
   communicator (RCCL or host), amgd_setup_device takes each rank's OWN entries (global
   indices; every rank's entries together are the matrix, duplicates summed in rank order),
   routes them to the owners of their rows (contiguous equal row blocks of level 0, every
   coarser level inheriting the owners), and builds a hierarchy of which each rank holds
   only its row blocks: rows of A, Af, W and AfP of every level and of every intermediate;
   products fetch the halo rows they reference, transposes exchange row pieces, vectors
   stay whole.  amgd_hier_export gathers the whole hierarchy to every rank (bit-identical
   to the one-GPU hierarchy).  amgd_comm_set_partitioned(1) after amgd_comm_init_* turns
   it on for amgd_setup_device; crs_setup with np > 1 runs partitioned unless
   amgd_comm_set_partitioned(0) chose the round-2 replicated mode; amg_setup always takes
   the whole matrix on the calling process (amg_setup.h:5) and runs the one-GPU setup
   there.  amgd_comm_free resets the choice. */
void amgd_comm_set_partitioned(int on);
int amgd_comm_partitioned(void);
/* Collective-consistency guard (also AMGD_COMM_CHECK=1): before every collective the
   ranks exchange (sequence number, kind, call site, sizes) and abort naming both ranks'
   call sites on a mismatch; an out-of-HBM on one rank inside a setup is announced the
   same way and every rank's setup returns -2 (without the guard it aborts the job).
   1 on, 0 off, -1 back to the environment.  amgd_comm_guard_calls: record exchanges so far. */
void amgd_comm_set_check(int on);
uint64_t amgd_comm_guard_calls(void);
/* scale of the per-op minimum work below which an op runs unsharded (1 = default, 0 = always shard) */
void amgd_comm_set_min_work(double scale);
void amgd_comm_stats(uint64_t *calls, uint64_t *bytes, double *ms);
void amgd_comm_stats_reset(void);

/* device scratch helpers for ctypes callers (bench/tests) */
void *amgd_dev_alloc(size_t bytes);
void amgd_dev_free(void *p);
void amgd_dev_upload(void *d, const void *h, size_t n);
void amgd_dev_download(void *h, const void *d, size_t n);
void amgd_dev_sync(void);                        /* wait for the library stream */

#ifdef __cplusplus
}
#endif
#endif
