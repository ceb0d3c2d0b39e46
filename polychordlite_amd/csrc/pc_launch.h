// pc_launch.h -- the host functions one .hip file of the engine defines and another calls, declared once.
//
// All of them have C linkage (tools and tests reach some by name), so a call through a stale hand-written prototype would link
// without a word: every file that defines or calls one includes this header, and the compiler compares each definition with it.
// Grouped by the file that defines them.  Launchers enqueue on stream `st` and do not wait.
#pragma once
#include "pc_state.h"
#include "../../include/polychord_hip.h"
#include <cstddef>
#include <memory>
#include <vector>

// What a device-source handle is (pc_rtc.hip keeps one per handle ever made, past pchip_source_destroy): the answer to every question the
// launchers, the engine and the doors have about a handle, asked once with pc_rtc_source_form.  All zero: no source, the plain form.
struct PcSourceForm {
    long nterms;                           // > 0: the terms form, the sum's length (a quadratic form: its nres)
    int nsums;                             // > 0: several sums per evaluation (pchip_source_create_sums)
    long nquad;                            // > 0: the quadratic form of that many residuals (pchip_source_create_quad): nterms == nquad
    long nshared;                          // > 0: shared values beside that form (pchip_source_create_shared)
    int has_prior;                         // the source defines pchip_prior_param as well (pchip_source_create_prior)
    long long ndata, ntail;                // the user's doubles, and the handle's own behind them in its block (a quadratic form's matrix)
    int alive;                             // 0: destroyed -- the launch shapes below still hold for a run in flight, nothing new starts on it
    int nbatch;                            // > 0: the BATCHED quadratic form of that many residuals (pchip_source_create_quad_batch, pc_quad_mm.hip): no
                                           // in-kernel evaluation -- nterms == nquad == 0, the LDS helpers below answer 0 --, its matrix in ntail as well
};

// A quadratic-form source keeps the residuals of the point -- of the two ends of a bracket -- in two blocks of nres doubles (an even
// number each: 16-byte reads) at the FRONT of the dynamic LDS of every kernel that evaluates the likelihood (pc_sample.hip, PC_DYN_LDS):
// their bytes; 0 for any other form
static inline size_t pc_quad_lds(const PcSourceForm &f) { return f.nquad > 0 ? sizeof(double) * 2 * (size_t)((f.nquad + 1) & ~1L) : 0; }

// The form's front block of that dynamic LDS: the quadratic form's two residual blocks, if any, then the two blocks of a handle with
// shared values (pchip_source_create_shared: nshared doubles a point, rounded up to even, for the two ends of a bracket).  Its bytes,
// which every launcher of a kernel that evaluates the likelihood adds to its own; 0 for any other form
static inline size_t pc_front_lds(const PcSourceForm &f) { return pc_quad_lds(f) + (f.nshared > 0 ? sizeof(double) * 2 * (size_t)((f.nshared + 1) & ~1L) : 0); }

// k_slice keeps the theta rows of a chain's babies in LDS (its run-time flag phi_lds: derived parameters at the end of the chain, summed
// in that order) when they fit under 48 KB next to the chain's block; pc_slice_t_ok takes only states where it does
// (pc_slice_plan's rule, asked by pc_slice_t_ok in another file: inline here, the one definition in this header, so that the library's
//  exported pc_* names stay what they were).  `f`: the form of the state's source, all zero for a state without one.  A source with several
// sums keeps the sums of every baby beside the rows, [nr][nsums]: the block counts here, and a shape it pushes over the limit writes its
// derived parameters inside the slice loop like any that does not fit.
// The front block of a quadratic form (pc_front_lds) counts in the same way.  A handle with shared values never takes the end-of-chain
// pass: there finish runs with lane = baby, and a lane has no shared block of its own -- its derived parameters are written inside the
// slice loop (like_phi_terms fills the point's block again), and its unit does not compile the lane = baby branch.
static inline int pc_slice_phi_lds(const PcState *S, const PcSourceForm &f)
{
    const size_t sh0 = sizeof(double) * ((size_t)S->D + S->nr) + 16, tb = sizeof(double) * (size_t)S->nr * (S->D + 1);
    const size_t sums = sizeof(double) * (size_t)S->nr * (size_t)f.nsums;
    if (f.nshared > 0) return 0;
    return (S->nDer > 0 && sh0 + tb + sums + pc_front_lds(f) <= 48 * 1024) ? 1 : 0;
}

extern "C" {

// ---- pc_abi.hip --------------------------------------------------------------------------------------------
// the text behind pchip_last_error (NULL clears)
void pc_abi_set_last_error(const char *msg);
// ---- pc_callback.hip ---------------------------------------------------------------------------------------
void pc_launch_slice_tick(const PcState *S, unsigned batch, int nchains, void *cs, double *x0s, int *decks, double *prop, const double *ev_logL,
                          const double *ev_theta, const double *ev_phi, int first, double *prop_host, int *need_host, hipStream_t st);
size_t pc_chain_state_size(void);
// the device batch callback's tick: answers read at rank[chain] of the dense blocks, nothing stored to the host
void pc_launch_slice_tick_dev(const PcState *S, unsigned batch, int nchains, void *cs, double *x0s, int *decks, double *prop, const double *ev_logL,
                              const double *ev_theta, const double *ev_phi, int first, const int *rank, hipStream_t st);
// ... for R runs of a group in step at once (grid.y = run; records with PC_REC_T_*, PC_REC_I_BATCH, PC_REC_I_FIRST).  1: not this way
int pc_launch_slice_tick_many(const PcManyRec *dR, int R, int nchains, hipStream_t st);
void pc_chain_need_layout(int *stride, int *offset);
// ---- pc_park.hip -------------------------------------------------------------------------------------------
// rank [nchains] (ascending enumeration of the chains with a flag, -1 without), their number to *count and *count_host (device-visible
// pinned word, or null), their cubes as rows of `cube` ([count][D]); flag of chain c at need[c * stride]
void pc_launch_park_pack(int nchains, int D, const int *need, int stride, const double *prop, int *rank, int *count, int *count_host,
                         double *cube, hipStream_t st);
// the pack of a group of nruns <= PC_PARK_MAX_RUNS runs into ONE block: runs[r] (device-visible) names run r's flags, proposals and rank array;
// rank: the GLOBAL row (the counts of the runs before + the run's own ascending enumeration, -1 without a flag); count [nruns] on the device;
// count_host [nruns + 1] (device-visible pinned words): each run's count, then the total; the cubes as rows of `cube` ([total][D]), run after
// run.  max_chains: the largest nchains among the runs.  1: not launched (nruns out of range)
int pc_launch_park_pack_many(int nruns, const PcParkRun *runs, int max_chains, int D, int *count, int *count_host, double *cube, hipStream_t st);
void pc_launch_live_cubes(const PcState *S, unsigned attempt0, int m, double *cube, hipStream_t st);
void pc_launch_live_gather(const PcState *S, int n, const int *idx, const double *cube, const double *theta, const double *phi,
                           const double *logL, double *rows, hipStream_t st);
// ---- pc_clus.hip -------------------------------------------------------------------------------------------
// 0: launched; 1: not this way (the caller takes the general kernel)
int pc_launch_killoff_cl(const PcState *S, int nc, hipStream_t st);
int pc_consume_cl_fits(const PcState *S, int nc);
// the kernel with parallel decisions: the same envelope, its own (larger) LDS block
int pc_consume_clp_fits(const PcState *S, int nc);
int pc_launch_consume_cl_many(const PcState *S, const PcManyRec *dR, int R, int wide, hipStream_t st);
int pc_launch_consume_cl(const PcState *S, int nc, hipStream_t st);
// ---- pc_cluster.hip ----------------------------------------------------------------------------------------
int pc_launch_knn_cluster_sub(const int *d_desc, int nb, int mmax, const double *Sm, const int *pool, int *knn, int *labels, int *out, hipStream_t st);
int pc_launch_knn_cluster_sub_many(const PcManyRec *dR, int R, int nb_max, int mmax, hipStream_t st);
void pc_launch_remap_chains(const PcState *S, const int *map, int nold, int n, hipStream_t st);
void pc_launch_shift_mats(const PcState *S, int p, int nc, hipStream_t st);
// (nd: descriptors, one per cluster; dims / ndims: the sub-dimension pass's coordinates, ndims = 0 the full space -- in the batched launchers below)
int pc_launch_knn_cluster_batch(const PcState *S, const int *h_desc, const int *d_desc, int nd, double *Sm, int *knn, int *labels, int *out, const int *dims, int ndims, hipStream_t st);
int pc_launch_knn_cluster_batch_dev(const PcState *S, const int *d_desc, int nd, int nmax, double *Sm, int *knn, int *labels, int *out, const int *dims, int ndims, hipStream_t st);
int pc_launch_knn_cluster_batch_many(const PcState *S, const PcManyRec *dR, int R, int nd_max, int nmax, int any_sub, hipStream_t st);
void pc_launch_rebuild(const PcState *S, int nc, hipStream_t st);
void pc_launch_ph_rehome(const PcState *S, int nph, int nc, const unsigned *old_uids, int nold_uids, int *counts, hipStream_t st);
// ---- pc_contract.hip ---------------------------------------------------------------------------------------
// use_rank: k_sort_live has run on this state in front of this launch
void pc_launch_nn_lists(const PcState *S, int nleft, int use_rank, hipStream_t st);
int pc_launch_nn_lists_many(const PcState *S, const PcManyRec *dR, int R, int nleft_max, int use_rank, hipStream_t st);
int pc_launch_consume(const PcState *S, int final_mode, int wide, hipStream_t st);
void pc_launch_init_state(const PcState *S, double logzero, hipStream_t st);
// ---- pc_rows.hip -------------------------------------------------------------------------------------------
void pc_launch_apply(const PcState *S, unsigned batch, int nchains, hipStream_t st);
// pool mode, a run on its own, deferred update: the row kernel and, in the same launch, the workgroups of the update's flag pass over nph rows
// (pc_upd_flag.h: keep [nph], blk [blocks of 256]), which also write the ids of the rows of the chains just consumed
void pc_launch_apply_flag(const PcState *S, unsigned batch, int nchains, int nph, unsigned char *keep, int *blk, hipStream_t st);
int pc_launch_apply_many(const PcState *S, const PcManyRec *dR, int R, unsigned batch, int nchains, hipStream_t st);
void pc_launch_install_live(const PcState *S, const double *rows, int n, hipStream_t st);
// ---- pc_update_steps.hip -----------------------------------------------------------------------------------
// phantom clean: returns nothing; *d_total (device int) receives the surviving count
void pc_launch_clean(const PcState *S, int nph, unsigned char *keep, int *blk, int *d_total, double *ph2, double *phL2, unsigned *phC2, unsigned long long *phU2, int *dst_index, hipStream_t st);
// ... for R runs at once: every run its own row count (PcManyRec::ia[PC_REC_I_ROWS], blocks PC_REC_I_BLOCKS)
int pc_launch_clean_many(const PcManyRec *dR, int R, int nblk_max, hipStream_t st);
void pc_launch_reset_thresholds(const PcState *S, hipStream_t st);
int pc_launch_reset_thresholds_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st);
int pc_cov_nchunk(const PcState *S, int nph);
int pc_launch_covmats(const PcState *S, int nph, int nc, double *psum, int *pcnt, double *mean, int *count, double *pcov, hipStream_t st);
// pieces of the general update path used by the fused update of pc_update.hip
void pc_launch_scan_blocks(int *blk, int nblk, int *total, int *total2, hipStream_t st);
void pc_launch_chol_only(const PcState *S, const double *ncov, const int *count, hipStream_t st);
int pc_post_blocks(void);
void pc_launch_post_moments(const PcState *S, int nd, double *pmax, double *part, hipStream_t st);
// ---- pc_engine.hip: Engine, pchip_run[_hooks], the option and cache entry points, the device maximiser (the kernel-level doors of the
//      tests, declared in polychord_hip.h, are pc_doors.h, which it includes) -----------------------------------------------------------
// called before several scheduler groups start on a device, while it is idle: the pool gets at least `want` streams
void pc_prepare_streams(int dev, int want);
// scratch blocks kept between calls (the driver works frees off for 10 ... 30 ms)
void *pc_cache_dev_alloc(size_t bytes);
void pc_cache_dev_free(void *p);
void *pc_cache_host_alloc(size_t bytes);
void pc_cache_host_free(void *p);
// several runs of one problem in step on a device.  Returns 0 or the first failing run's code.
int pc_run_many(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nseeds, const int *seeds, int device, int max_in_flight, pchip_result *results);
// A source likelihood under a HOST prior (the PolyChord-interface doors): an evaluator opened once per run -- the handle's data block resident
// on `device`, a stream and buffers of its own -- whose pc_source_batch_eval is a polychord_batch_fn (user = the evaluator): the host prior
// row by row on the calling thread, then one launch of k_source_eval for all n rows.  open: NULL with the reason in polychord_hip_last_error()
void *pc_source_batch_open(int handle, int device, int nDims, int nDerived, polychord_prior_fn prior);
void pc_source_batch_eval(void *user, int n, int nDims, int nDerived, const double *cube, double *theta, double *phi, double *logL);
void pc_source_batch_close(void *user);
// the batch callback registered now (polychord_hip_set_batch_callback)
void pc_batch_callback_get(polychord_batch_fn *fn, void **user);
int pc_device_batch_registered(void);
// ---- pc_fast.hip -------------------------------------------------------------------------------------------
// _fits: 1 where the kernel's LDS block fits; launchers: 0: launched; 1: not this way
int pc_fast_fits(const PcState *S);
int pc_launch_sort_live(const PcState *S, hipStream_t st);
int pc_launch_sort_live_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st);
int pc_launch_consume_fast(const PcState *S, int final_mode, hipStream_t st);
void pc_launch_ph_prepare(const PcState *S, hipStream_t st);
// ---- pc_merge.hip ------------------------------------------------------------------------------------------
// the lived records of a run packed on its device into `block`: rows [cap][nT] | entry [cap] | own log weight [cap] | scratch
size_t pc_records_block_bytes(long long cap, int nT);
int pc_pack_lived_device(const double *dead, const double *logw, const double *entry, long long nd, int nT, double logzero, double *block, long long cap, long long *h_count, hipStream_t st);
// ---- pc_par.hip --------------------------------------------------------------------------------------------
// _fits: 1 where the kernel's LDS block fits; launchers: 0: launched; 1: not this way
int pc_par_fits(const PcState *S);
int pc_launch_consume_par(const PcState *S, hipStream_t st);
// the same launch for R runs of one shape at once (blockIdx.y = run; dR: device array of their records)
int pc_launch_consume_par_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st);
// the contraction's binary search, ranks and acceptance alone, on the keys of given logL (device arrays: snap [n] ascending, cand [T] by step,
// valid [T] -> accept [T]; serial: the acceptance of settings.ablate bit 18).  0: launched; 1: not these sizes (n <= 8192, T <= 1024)
int pc_launch_par_accept(int n, const double *snap, int T, const double *cand, const unsigned char *valid, int serial, unsigned char *accept,
                         hipStream_t st);
// the one-cluster kill-off whole (the rows moved inside: runs in step) / split for a run on its own: k_final_par without its row loop, k_final_rows behind it
int pc_launch_final_par(const PcState *S, hipStream_t st);
int pc_launch_final_par_split(const PcState *S, hipStream_t st);
int pc_launch_final_par_many(const PcManyRec *dR, int R, hipStream_t st);
// ---- pc_rtc.hip --------------------------------------------------------------------------------------------
// launched by PC_LAUNCH (pc_sample.hip) with the variant, grid, block, dynamic LDS and arguments the launcher chose for the static kernel.
// 0: launched; 1: no such kernel (pc_rtc_error has the text)
int pc_rtc_launch(const PcState *S, const char *expr, dim3 grid, dim3 block, size_t sh, hipStream_t st, void **args);
const char *pc_rtc_error(void);
// the form of handle `id` in *f (zeroed first): one lock, one lookup.  0, or non-zero for an id that never existed; a destroyed handle
// answers what it answered alive, with alive = 0
int pc_rtc_source_form(int id, PcSourceForm *f);
// ---- pc_quad_mm.hip ----------------------------------------------------------------------------------------
// The batched quadratic form (pchip_source_create_quad_batch): chi2 of n rows at once on the matrix cores, between the two run-time kernels
// that call the user's functions (k_quad_residuals, k_quad_finish: pc_sample.hip under PCHIP_USER_QUAD_BATCH).  All sizes are functions of
// nres alone: ldr, the leading dimension of the residual block (nres rounded up to 16); ncb, the partial sums a row (one per wavefront's
// strip of 32 columns).  Rows come in blocks of PC_QUAD_MM_ROWS: the scratch holds pc_quad_mm_rows(n) of them, padding rows zero.
#define PC_QUAD_MM_ROWS 64
static inline int pc_quad_mm_ldr(int nres) { return (nres + 15) & ~15; }
static inline int pc_quad_mm_ncb(int nres) { return 4 * ((nres + 127) / 128); }
static inline long pc_quad_mm_rows(long n) { return (n + PC_QUAD_MM_ROWS - 1) / PC_QUAD_MM_ROWS * PC_QUAD_MM_ROWS; }
// the most rows one evaluation takes (the callers cut longer blocks into slabs: a row's bits do not depend on the cut); R is 256 MB at the
// largest nres then
#define PC_QUAD_BATCH_SLAB 8192
// k_quad_chi2_mm: R [pc_quad_mm_rows(n)][ldr] (device), P [nres][nres] row-major exactly as given, part [pc_quad_mm_rows(n)][ncb].  1: not launched
int pc_launch_quad_chi2_mm(int n, int nres, const double *R, const double *P, double *part, hipStream_t st);
// the whole evaluation of n rows (device pointers; S: a source state of the handle -- like.kind, src_id, src_data, src_ndata, D, nDer):
// residuals, chi2, finish, three launches on `st`; R / part: scratch for pc_quad_mm_rows(n) rows.  1: not launched (pc_rtc_error, or the
// text behind pchip_last_error)
int pc_launch_quad_batch(const PcState *S, int nres, int n, const double *thetas, double *logL, double *phi, double *R, double *part, hipStream_t st);
// why a likelihood / prior pair is refused where a batched handle is involved (NULL: it is not, or the likelihood is no batched handle);
// `who`: the entry point's name.  *nres (may be NULL): the handle's residuals, 0 for any other likelihood.  Before any device call
const char *pc_quad_batch_refusal(const char *who, const pchip_like *like, const pchip_prior *prior, int *nres);
// ---- pc_bases.hip ------------------------------------------------------------------------------------------
// The launchers of the direction kernels (static kernels only): 0: launched; 1: not this way (no kernel for this shape).
// the split launch (see k_nhats): part 1 = bases, part 2 = seeds + whitening; 1 where it exists (else only the whole kernel: pc_launch_nhats)
int pc_nhats_splittable(const PcState *S);
// packed (part 1, nDims <= 24; where its kernel does not take the state, k_nhats<.., 1>): which kernel draws the bases -- the same bits from each
enum { PC_PART1_BASIS = 0,      // k_nhats<.., 64, 1>: a wavefront a basis (graded runs; settings.ablate bit 19)
       PC_PART1_PACKED = 1,     // k_deviates_t + k_bases_packed of pc_slice_t.hip (runs in step; settings.ablate bit 7), no deck records
       PC_PART1_WAVE = 2 };     // k_nhats_w: 64 / nDims bases a wavefront, one launch, deck records (a run on its own, one grade)
// (the one place that says which: `packed` is pc_plan.h's decision for the nursery, or bit 7 on the side stream)
static inline int pc_part1_kind(bool packed, int ablate) { return packed ? PC_PART1_PACKED : ((ablate & PC_ABL_BASES_WAVE) ? PC_PART1_BASIS : PC_PART1_WAVE); }
int pc_launch_nhats_part(const PcState *S, unsigned batch, int nchains, int part, hipStream_t st, int packed);
int pc_launch_nhats(const PcState *S, unsigned batch, int nchains, hipStream_t st);
// ... and for R runs of a device in step (grid.z = run) the shapes that do not split: 24 < nDims <= 64
int pc_launch_nhats_many(const PcState *S, const PcManyRec *dR, int R, int nchains, hipStream_t st);
// ---- pc_sample.hip -----------------------------------------------------------------------------------------
// Launchers: 0: launched; 1: not this way (no kernel for this shape, or the run-time module failed: pc_rtc_error).
// the sampling kernels come from the run-time module (a source likelihood, settings.ablate bit 15)
int pc_rtc_wanted(const PcState *S);
int pc_launch_generate_live(const PcState *S, int attempt0, int n, double *rows, double *rows_logL, hipStream_t st);
// 1: k_slice can do seeds + whitening itself (pc_launch_slice_fused; pc_launch_slice_many with fused = 1)
int pc_slice_fusable(const PcState *S);
int pc_launch_slice_fused(const PcState *S, unsigned batch, int nchains, hipStream_t st);
// R runs of a device in step (grid.y = run, every run the same shape).  1: a shape only the one-run launchers take
int pc_launch_slice_many(const PcState *S, const PcManyRec *dR, int R, int nchains, int fused, hipStream_t st);
// ... where the problem is the user's own -- a source likelihood, a prior table, a source prior --: the general variants with the prior kind
// as a template argument and the terms form's LDS (a table of its own behind pc_slice_launch).  1: no shared launch for this shape (nDims > 64
// unfused, grades, the sequential stream, the correlated Gaussian): each run then launches its own k_slice
int pc_launch_slice_step(const PcState *S, const PcManyRec *dR, int R, int nchains, int fused, hipStream_t st);
int pc_launch_slice(const PcState *S, unsigned batch, int nchains, hipStream_t st);
// pchip_prior_transform: the device transform of the table in S->prior at n points (device pointers); the device batch callback's prior:
// a table, or the uniform box (S->prior.kind 1, lo / hi or null) as k_generate_live forms it
int pc_launch_prior_transform(const PcState *S, int n, const double *cubes, double *thetas, hipStream_t st);
// pchip_source_eval: a source likelihood at n points (device pointers), by the handle's run-time module
int pc_launch_source_eval(const PcState *S, int n, const double *thetas, double *logL, double *phi, hipStream_t st);
// the prior of a source handle (prior.kind 3) at n points: k_prior_transform by name from the handle's module
int pc_launch_source_prior_eval(const PcState *S, int n, const double *cubes, double *thetas, hipStream_t st);
// the device maximiser (nDims <= 64; static kernels, or by name from the run-time module: a source handle, settings.ablate bit 15).
// k_max_rank: val[i] = logL_i + dXdtheta(cube_i) of n live rows [n][nT].  k_maximise: nprob problems, one wavefront each -- in: nprob records
// of (D + 1) D start cubes | D + 1 values | D + nDer posterior mean; hdr: leg (0 likelihood, 1 posterior) and has-mean per problem; out: nprob
// records of 2 D + 2 nDer + 4 doubles [cube | theta | phi | logL | dXdtheta | logL(mean) | value | phi(mean)]; outi: iterations and likelihood calls
int pc_launch_max_rank(const PcState *S, int n, const double *rows, double *val, hipStream_t st);
int pc_launch_maximise(const PcState *S, int nprob, const double *in, const int *hdr, long long max_iter, double *out, long long *outi, hipStream_t st);
// ---- pc_maximise.hip ---------------------------------------------------------------------------------------
// do_maximisation's choice of simplex (maximiser.F90:92-161), the one copy both maximisers use: per cluster with at least D + 1 rows the D + 1
// best by stable sort of `vals` (NULL: the rows' logL), the cluster whose best value is strictly highest, in index order, wins.  simplex
// [(D + 1) D] and f [D + 1] are filled ascending; returns the cluster, or -1: no simplex can be built
int pc_max_choose_simplex(int nDims, int nTotal, double logzero, const double *live, const int *cluster, int nlive, const double *vals,
                          double *simplex, double *f);
// the three point arrays of a pchip_maximum (zeroed first), for pchip_maximum_free
void pc_maximum_alloc(pchip_maximum *m, int nDims, int nDerived);
// ---- pc_slice_t.hip ----------------------------------------------------------------------------------------
// lane = chain / lane = basis.  _ok: 1 where the kernels take the state; launchers: 0: launched; 1: not this way
int pc_bases_t_ok(const PcState *S);
int pc_launch_bases_t(const PcState *S, unsigned batch, int nchains, hipStream_t st);
int pc_launch_bases_t_many(const PcState *S, const PcManyRec *dR, int R, unsigned batch, int nchains, hipStream_t st);
int pc_slice_t_ok(const PcState *S, int ncluster);
int pc_launch_slice_t(const PcState *S, unsigned batch, int nchains, hipStream_t st);
int pc_launch_slice_t_many(const PcState *S, const PcManyRec *dR, int R, unsigned batch, int nchains, hipStream_t st);
// ---- pc_update.hip -----------------------------------------------------------------------------------------
// the fused update: _ok 1 where it exists (one cluster, nDims <= 128)
int pc_update_fused_ok(const PcState *S, int nc);
int pc_update_fused_blocks(const PcState *S, int nph);
int pc_update_fused_entries(const PcState *S);
// nph >= 1.  keep [nph], blk [blocks], part [pc_update_fused_blocks * pc_update_fused_entries] doubles, shift [D]; deferred: see k_upd_flag.
// d_total [PC_UPD_CTR_INTS]: the survivor count and, behind it, the ticket counters of the two-launch chain (settings.ablate bit 16) -- zero
// when first handed in (the chain leaves them zero)
#define PC_UPD_CTR_INTS 2048
void pc_launch_update_fused(const PcState *S, int nph, unsigned char *keep, int *blk, int *d_total, double *ph2, double *phL2, unsigned *phC2,
                            unsigned long long *phU2, double *part, double *shift, int deferred, hipStream_t st);
// ... flagged: keep and blk were made for these nph rows by pc_launch_apply_flag in front (pool mode, deferred, not the chain): no k_upd_flag
void pc_launch_update_fused_at(const PcState *S, int nph, unsigned char *keep, int *blk, int *d_total, double *ph2, double *phL2, unsigned *phC2,
                               unsigned long long *phU2, double *part, double *shift, int deferred, int flagged, hipStream_t st);
int pc_update_fused_grid(const PcState *S, int nph, int deferred);
// ... for R runs, all of them the same number G of gathering workgroups (pc_update_fused_grid) and nblk_max >= their blocks.
// 1: not this way (the caller launches them one by one)
int pc_launch_update_fused_many(const PcState *S, const PcManyRec *dR, int R, int nblk_max, int G, int deferred, hipStream_t st);

}   // extern "C"

// ---- pc_rtc.hip, C++ linkage ---------------------------------------------------------------------------------
// A hold on the data block of a LIVE handle (the user's f->ndata doubles, then f->ntail of the handle's own; its form in *f where f is not
// NULL), or nullptr: the handle does not exist, or was destroyed.  The block lives as long as any hold does, whatever happens to the
// handle: a caller keeps its hold until its copy to pinned or device memory has been issued from it.
std::shared_ptr<const std::vector<double>> pc_rtc_source_hold(int id, PcSourceForm *f);
