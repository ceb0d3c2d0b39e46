/*
 * polychord_hip.h -- C ABI of libpolychord_hip.so, the MI355X-native nested-sampling engine
 * that is a drop-in behind PolyChordLite's own C boundary.
 *
 * Part 1 re-declares, symbol for symbol, what the reference exports from its Fortran
 * ISO_C_BINDING shim (reference src/polychord/interfaces.h:2-56, implemented in
 * src/polychord/interfaces.F90:285-436 and :496-519).  A caller linked against the
 * reference's libchord.so links against libpolychord_hip.so unchanged.
 *
 * Part 2 is the engine's own plain-C surface (no torch types, plain pointers and sizes): device
 * likelihood selectors, the batched engine entry used by bench.py / tests, and kernel-level entry
 * points for parity tests.
 */
#ifndef POLYCHORD_HIP_H
#define POLYCHORD_HIP_H
#include <stdbool.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ===== Part 1: the reference's C boundary ================================================== */

/* loglikelihood(theta, nDims, phi, nDerived) -> logL      (interfaces.h:3, interfaces.F90:291-300) */
typedef double (*polychord_loglike_fn)(double *theta, int nDims, double *phi, int nDerived);
/* prior(cube, theta, nDims): hypercube -> physical        (interfaces.h:4, interfaces.F90:302-309) */
typedef void (*polychord_prior_fn)(double *cube, double *theta, int nDims);
/* dumper(ndead, nlive, npars, live, dead, logweights, logZ, logZerr)
 *                                                          (interfaces.h:5, interfaces.F90:311-322) */
typedef void (*polychord_dumper_fn)(int ndead, int nlive, int npars, double *live, double *dead,
                                    double *logweights, double logZ, double logZerr);

/* replaces polychord_c_interface (interfaces.h:2-45, interfaces.F90:285-436).  Scalars by value,
 * `comm` by reference (an MPI_Fint in the reference's MPI build; ignored here, ranks are processes
 * of torch.distributed / one GPU each).  Strings are NUL-terminated. */
void polychord_c_interface(
    polychord_loglike_fn loglikelihood, polychord_prior_fn prior, polychord_dumper_fn dumper,
    int nlive, int num_repeats, int nprior, int nfail, bool do_clustering, int feedback,
    double precision_criterion, double logzero, int max_ndead, double boost_posterior,
    bool posteriors, bool equals, bool cluster_posteriors, bool write_resume, bool write_paramnames,
    bool read_resume, bool write_stats, bool write_live, bool write_dead, bool write_prior,
    bool maximise, double compression_factor, bool synchronous, int nDims, int nDerived,
    char *base_dir, char *file_root, int nGrade, double *grade_frac, int *grade_dims, int n_nlives,
    double *loglikes, int *nlives, int seed, int *comm);

/* replaces polychord_c_interface_ini (interfaces.h:47-56, interfaces.F90:496-519) */
void polychord_c_interface_ini(polychord_loglike_fn loglikelihood, void (*setup_loglikelihood)(void),
                               char *inifile, int *comm);

/* ===== Part 2: engine surface =============================================================== */

enum { PCHIP_LIKE_CALLBACK = 0, PCHIP_LIKE_GAUSSIAN = 1, PCHIP_LIKE_RASTRIGIN = 2,
       PCHIP_LIKE_TWIN_GAUSSIAN = 3, PCHIP_LIKE_CORR_GAUSSIAN = 4, PCHIP_LIKE_SOURCE = 5 };

/* Built-in likelihoods that run fused on the device.  These are ordinary host functions with the
 * reference's callback signature (they evaluate the same formula on the host); when one of them
 * is passed as `loglikelihood` to polychord_c_interface the engine recognises the pointer and
 * evaluates the likelihood inside the slice-sampling kernel instead of calling back.
 * (likelihoods/examples/gaussian.f90:12-41, rastrigin.f90:20-35, twin_gaussian.f90:14-56,
 *  random_gaussian.f90:17-30) */
double polychord_hip_gaussian(double *theta, int nDims, double *phi, int nDerived);
double polychord_hip_rastrigin(double *theta, int nDims, double *phi, int nDerived);
double polychord_hip_twin_gaussian(double *theta, int nDims, double *phi, int nDerived);
double polychord_hip_corr_gaussian(double *theta, int nDims, double *phi, int nDerived);
/* parameters of the built-ins (process-global like the reference's setup_loglikelihood state) */
void polychord_hip_set_gaussian(double mu, double sigma);
void polychord_hip_set_corr_gaussian(int nDims, const double *invcov_rowmajor, const double *mean, double logdetcov);
/* uniform box prior evaluated on the device; pass polychord_hip_uniform_prior as `prior` */
void polychord_hip_uniform_prior(double *cube, double *theta, int nDims);
void polychord_hip_set_uniform_prior(int nDims, const double *lo, const double *hi);
/* The reference's prior types as a table, evaluated INSIDE the sampling kernels when the likelihood is a device likelihood: one entry
 * per PARAMETER -- the type number of priors.f90:5-15, the prior block, the prior parameters in the ini file's order -- and the
 * hypercube index of every parameter (priors.f90:708-737; NULL = identity).  sorted_ blocks are consecutive parameters of one type
 * and block (priors.f90:245-262).
 * The adaptive types 11-15 (priors.f90:363-488) are blocks of consecutive parameters of one type and block as well.  With x_1 .. x_n the
 * block's cube coordinates:
 *   adaptive_sorted_{uniform, gaussian, half_gaussian, exponential}, n >= 2: parameter 1 is the count, theta_1 = 0.5 + x_1 (n - 1), not
 *     rounded.  nfunc = INT(theta_1 + 0.5); parameters 2 .. nfunc+1 are sorted among themselves like a sorted_ block of nfunc, parameters
 *     nfunc+2 .. n keep y = x, and parameters 2 .. n go through the base transform, each with its own prior parameters.
 *   nn_adaptive_layer_gaussian, n >= 3: parameter 1 is the layer number, theta_1 = 0.5 + 2 x_1; parameters 2 .. n are an adaptive block
 *     of n - 1 (its count is parameter 2) whose base is half_gaussian where theta_1 < 1.5 and gaussian otherwise.
 *   EVERY parameter of such a block, the count and the layer included, gives exactly the base type's number of prior parameters (2; 1 for
 *     exponential): the reference skips the count's by position.  The count's and the layer's values are read and ignored.
 *   One defined deviation: for x_1 = 1 - 2^-53 and n - 1 a power of two the reference's nfunc comes out as n and it sorts one element
 *     past its array; here nfunc is clamped to 1 .. n-1, on the host and on the device. */
enum { PCHIP_PT_UNIFORM = 1, PCHIP_PT_LOG_UNIFORM = 2, PCHIP_PT_POWER_UNIFORM = 3, PCHIP_PT_GAUSSIAN = 4, PCHIP_PT_HALF_GAUSSIAN = 5,
       PCHIP_PT_EXPONENTIAL = 6, PCHIP_PT_SORTED_UNIFORM = 7, PCHIP_PT_SORTED_GAUSSIAN = 8, PCHIP_PT_SORTED_HALF_GAUSSIAN = 9,
       PCHIP_PT_SORTED_EXPONENTIAL = 10, PCHIP_PT_ADAPTIVE_SORTED_UNIFORM = 11, PCHIP_PT_ADAPTIVE_SORTED_GAUSSIAN = 12,
       PCHIP_PT_ADAPTIVE_SORTED_HALF_GAUSSIAN = 13, PCHIP_PT_ADAPTIVE_SORTED_EXPONENTIAL = 14, PCHIP_PT_NN_ADAPTIVE_LAYER_GAUSSIAN = 15 };
typedef struct {
    int type;                      /* PCHIP_PT_* */
    int block;                     /* prior block (the ini file's fifth column); only tells sorted_ and adaptive blocks of one type apart */
    int npar;                      /* prior parameters given (uniform, log_uniform, gaussian, half_gaussian: 2; exponential: 1; power_uniform: 3) */
    double par[3];
} pchip_prior_entry;
/* polychord_hip_table_prior is a real host function (the maximiser, write_prior, tests and a reference-side caller evaluate it); passed
 * as `prior` to polychord_c_interface with a built-in likelihood the engine recognises the pointer and evaluates the table on the
 * device.  polychord_hip_set_table_prior checks the table: 0, or non-zero with the message in polychord_hip_last_error(). */
void polychord_hip_table_prior(double *cube, double *theta, int nDims);
int  polychord_hip_set_table_prior(int nDims, const pchip_prior_entry *entries, const int *hyper);
/* A likelihood (and prior) written as device source -- pchip_source_create and its kin in Part 2 below, any form -- behind the reference's
 * callback signatures.  polychord_hip_set_source names the handle the next polychord_c_interface / _ini calls use (sticky and
 * process-global like polychord_hip_set_gaussian; 0 clears it): 0, or non-zero with "... handle N does not exist" in
 * polychord_hip_last_error().  The handle must be alive when the run starts.  Passed as `loglikelihood`, polychord_hip_source_loglike
 * is recognised like a built-in: the handle is evaluated inside the sampling kernels under polychord_hip_uniform_prior, under
 * polychord_hip_table_prior (so under any ini prior block) and under polychord_hip_source_prior, the handle's own pchip_prior_param
 * (pchip_source_create_prior; only with polychord_hip_source_loglike as the likelihood); `maximise` then polishes on the device
 * (pchip_maximise_device; nDims > 64 or no simplex: a message, no file).  Under any other prior function -- the caller's own -- the prior
 * is called on the host, on the calling thread, and the parked proposals of a round are evaluated by ONE launch of the source (unless the
 * caller registered a batch callback, which is then used as always).
 * Both are also real host functions: pchip_source_eval / pchip_source_prior_eval at one point, the same bits -- ONE kernel launch a call,
 * for single evaluations (a script calling its likelihood, cube_samples), not a sampling path.  Without a handle set, or for
 * polychord_hip_source_prior with a handle that defines no prior, they end like a fatal condition of polychord_c_interface: message and
 * `stop 1`, or in "halt_returns" mode the message in polychord_hip_last_error() and a return (logL then below any logzero). */
int  polychord_hip_set_source(int handle);
double polychord_hip_source_loglike(double *theta, int nDims, double *phi, int nDerived);
void polychord_hip_source_prior(double *cube, double *theta, int nDims);
/* Batched host evaluation.  In host-callback mode the engine parks the proposals of all chains of a nursery and hands them
 * to the host together; with a batch callback registered it makes ONE call per round instead of one loglikelihood call
 * per proposal: prior + likelihood for n hypercube points (row-major, host memory; logL[i] <= logzero marks an invalid
 * point).  This is the hook for vectorised likelihoods, for likelihoods that run on an accelerator themselves, and for
 * farming the evaluations out to MPI ranks (what the reference's MPI workers did, nested_sampling.F90:426-498).  The scalar
 * callbacks passed to polychord_c_interface must still be valid (they serve the maximiser and single evaluations).
 * Process-global like the other setters; NULL removes it. */
typedef void (*polychord_batch_fn)(void *user, int n, int nDims, int nDerived, const double *cube, double *theta, double *phi,
                                   double *logL);
void polychord_hip_set_batch_callback(polychord_batch_fn fn, void *user);
/* The batch callback for likelihoods that already live on the GPU (a tensor program, a pipeline of library calls): the parked proposals
 * of a round are packed into one dense block in DEVICE memory, in ascending chain order, and the answers are read where the callback
 * wrote them -- no row visits the host; the host reads one int per round.
 * flags bit 0: d_theta already holds the prior transform of d_cube (the run's prior is the box or a table: evaluated by the engine
   on the device); otherwise the callback writes d_theta from d_cube, as the host batch callback does.
   All pointers are device memory of the run's device, row-major, dense: cube, theta [n][nDims], phi [n][max(1,nDerived)], logL [n].
   stream: the engine's hipStream_t.  On return the callback's work is either complete or enqueued on `stream` (work on another
   stream: make `stream` wait for it, or synchronise, before returning).  logL[i] <= logzero marks an invalid point.
   The blocks are valid in the order of `stream` as well: what fills them (the live points' draws, the engine's prior) may still be
   running when the callback is entered, so work that is NOT enqueued on `stream` -- a blocking hipMemcpy included -- first waits for it.
   Returns 0; non-zero ends the run like polychord_hip_request_stop.
 * Process-global and sticky like the host batch callback, read when a run starts; NULL removes it.  Only in callback mode
 * (like.kind == PCHIP_LIKE_CALLBACK) of pchip_run / pchip_run_hooks and the doors on top of them; with both batch callbacks registered this
 * one wins.  The scalar callbacks must still be valid (the maximiser, cube_samples, single evaluations).  prior.kind 0 (a host function):
 * the callback owns the prior, flags 0; prior.kind 1 / 2: the engine's transform, the bits of the sampling kernels' box and of
 * pchip_prior_transform, flags 1 (nDims <= 256); prior.kind 3 stays refused with a callback likelihood.  The live points are drawn on the
 * device from the Philox coordinates of the host path, so a run is the host batch callback's run of the same functions.
 * pchip_result.path[PCHIP_PATH_DEVICE_BATCH] counts the calls.
 * Several seeds in step (pchip_run_in_step with like.kind == PCHIP_LIKE_CALLBACK while this callback is registered): ONE call a tick for the
 * parked proposals of all runs of a group.  The rows are ordered by run (the order of `seeds` within the group) and inside a run by
 * ascending chain: the solo order, concatenated; the callee is not told where one run's rows end.  flags, the stream rule, the return code
 * and logzero are as above; a non-zero return stops every run of the group (code 5).  The callee is always called on the thread that called
 * pchip_run_in_step.  Each run is bit for bit its solo pchip_run through the same callback PROVIDED the callee's answer for a row depends
 * neither on the row's position in the block nor on n -- a batched product that rounds by row position (see pc_park.hip) gives runs that
 * differ from the solo ones in the last bits, and whatever follows from those. */
typedef int (*polychord_device_batch_fn)(void *user, int n, int nDims, int nDerived, const double *d_cube, double *d_theta,
                                         double *d_phi, double *d_logL, int flags, void *stream);
void polychord_hip_set_device_batch_callback(polychord_device_batch_fn fn, void *user);
/* asks a running engine to stop at the next host callback boundary (used by language bindings when a
 * user callback raised: the reference throws through the Fortran frames, _pypolychord.cpp:219-224) */
void polychord_hip_request_stop(void);
/* .resume files (reference grammar) without a run: parse `in`, optionally write it back to `out`;
 * counts[0..5] = nDims, nDerived, ndead, ncluster, ncluster_dead, total live points.  0 on success. */
int polychord_hip_resume_copy(const char *in, const char *out, int *counts);
/* the prior block of an ini file (ini.f90:354-458, priors.f90: uniform, log_uniform, power_uniform, gaussian,
 * half_gaussian, exponential and their sorted_ variants) evaluated at one hypercube point; returns nDims, -1 if n < nDims */
int polychord_hip_ini_prior(const char *inifile, const double *cube, double *theta, int n);
/* inverse normal CDF, AS241 PPND16 (utils.F90:806-966) */
double polychord_hip_inv_normal_cdf(double p);
/* engine options by name: "batch" (chains per nursery), "device" (HIP device ordinal), "halt_returns" (1: a fatal
 * condition inside polychord_c_interface -- which the reference answers with a message and `stop 1`, abort.F90:19-29,
 * and so does this library by default -- returns to the caller instead, with the message kept for
 * polychord_hip_last_error(): what a language binding needs to raise an exception rather than lose its interpreter),
 * "inject_fault" (tests: the next run fails once -- 1: a device allocation, 2: cluster capacity at the next split,
 * 3: growth of the phantom array), "device_prior" (default 1; 0: polychord_c_interface_ini and polychord_hip_table_prior evaluate
 * their prior table on the host as before -- a built-in likelihood then runs as a host callback too) */
void polychord_hip_set_option(const char *name, double value);
/* sub-dimension clustering of the next polychord_c_interface calls (sticky, like the options above): n 0-based hypercube
 * indices (pchip_settings.sub_cluster_dims); n = 0 clears it.  polychord_c_interface_ini sets the ini file's markers for
 * its own call and restores this setting afterwards. */
void polychord_hip_set_sub_clustering(int n, const int *dims);
/* the sub-clustering list of an ini file (parameters whose name holds a `*`, ini.f90:389-393; priors.f90:740-741): the
 * 0-based hypercube indices in parameter order, at most `cap` of them written to dims; returns how many there are */
int polychord_hip_ini_sub_clustering(const char *inifile, int *dims, int cap);
/* message of the fatal condition that ended the last polychord_c_interface call in "halt_returns" mode, else NULL */
const char *polychord_hip_last_error(void);
void pchip_inject_fault(int kind);
/* initial capacities of the per-cluster arrays (default 128) and of the phantom array (rows; 0 = estimate); both grow on
   demand like the reference's reallocating arrays (run_time_info.f90:392-418), options "cluster_capacity" / "phantom_capacity" */
void pchip_set_capacity(int clusters, int phantom_rows);
/* The engine keeps the device and pinned blocks of finished runs for the next ones (up to 64 GB / 12 GB); this gives them back
 * to the driver -- e.g. after many runs in flight, before a run that sizes its buffers by the memory that is free.
 * polychord_hip_set_option("trim_cache", 0) does the same. */
void pchip_trim_cache(void);
/* How many device and pinned blocks the two caches have obtained from the driver and somebody holds now (a run in flight, a result
 * that has not been freed, the merge's scratch): equal before and after a call that gave back everything it took.  Either may be NULL. */
void pchip_blocks_in_use(long *device, long *pinned);

typedef struct {
    int nDims, nDerived;
    int nlive, num_repeats, nprior, nfail;
    int do_clustering;
    double precision_criterion, logzero;
    int max_ndead;
    double boost_posterior;
    int posteriors, equals, cluster_posteriors;
    double compression_factor;
    int n_nlives; const double *loglikes; const int *nlives;
    int seed;
    int batch;          /* chains per synchronous nursery (the reference's nprocs-1); 0 = auto */
    int device;         /* HIP device ordinal, -1 = current/0 */
    int feedback;
    int profile;        /* 0: off; 1: HIP-event stopwatch around every kernel class; otherwise a bit mask,
                           bit k+1 = time kernel class k (0 nhats, 1 slice, 2 consume, 3 apply, 4 clean, 5 covmats, 6 side-stream bases):
                           a few hundred event records per run instead of a few thousand; bits 8..15 = n: only every
                           n-th launch of a class is timed (k_launches then counts the timed ones) */
    int force_general;  /* 1: always use the general contraction kernel (tests) */
    int ablate;         /* developer / test switches, 0 = product: bit 0 = built-in quadratic likelihoods evaluated like a general functor;
                           bits 1, 2, 3 = no pool mode, no deferred update, no fused update (identical results by the older kernels);
                           bit 4 = evidence prefixes of the parallel contraction by pair scans only; bit 5 = several clusters: every
                           launch by the general contraction kernel (no one-wave kernel); bits 6, 7 = a run on its own by the kernels it uses
                           next to other runs of its device (bit 6: lane-per-chain sampling, pc_slice_t.hip; bit 7: lane-per-vector bases); bit 8 = the one-wave
                           contraction of clustered runs ends its launch at a cluster's death (the host relaunches for the rest of the nursery) instead
                           of sorting the live set itself and going on; bit 9 = the kill-off of a run that ends with several clusters by the general
                           contraction kernel instead of the one-wave kernel k_killoff_cl (the same bits); bit 10 = several clusters: the contraction whose ONE
                           wavefront decides chain after chain (k_consume_cl) instead of the one with parallel decisions (k_consume_clp): the same run; bits 11, 12 = retired,
                           no effect (experiments that were removed, CHANGELOG.md); bit 13 = the
                           fused sampling kernel with ONE wavefront a workgroup (a chain) instead of four chains and their four helper wavefronts
                           (deck shuffle and whitening next to the seed choice instead of in front of it): the same numbers; bit 14 = with the helper, the closed
                           form's s.M.s of a direction reduced by the chain at the head of its slice instead of taken from the table the helper made with the
                           whitening (the same bits: the table's sums follow the wave butterfly's order); bit 15 = the sampling kernels of the built-in
                           likelihoods launched from a module compiled at run time (pchip_source_create's path, PCHIP_PATH_SOURCE_KERNELS): the same numbers; bit 16 = the
                           one-cluster update as a chain of two launches whose last-arriving workgroups go on with the next stage (pc_update.hip)
                           instead of five launches (flag, index, gather, fold, final): the same rows in the same order and the same groups of
                           sums, the same bits; slower at the metric configuration, kept as the independent second way the tests compare with;
                           bit 17 = a run on its own in pool mode: the update's flags by k_upd_flag in a launch of its own behind the row kernel
                           instead of by workgroups of the row kernel's launch (k_apply_pool_flag): the same bits; bit 18 = the parallel
                           contraction's acceptance as the serial recurrence, sixty-four steps at a time on one wavefront, instead of one dominance
                           count a step for all steps at once (pc_par.hip): the same bits; bit 19 = a run on its own, nDims <= 24, one grade:
                           the orthonormal bases by the kernel with a wavefront a basis (k_nhats) instead of 64 / nDims bases a wavefront
                           (k_nhats_w, pc_bases.hip): the same bits; bit 20 = ... k_nhats_w with one wavefront a workgroup instead of four
                           (three more that share the deviates and make the decks): the same bits */
    const char *resume_write;  /* path of a .resume file (reference grammar, read_write.F90:219-288) rewritten at every
                                  update and at the end; NULL = off */
    int sequential_rng; /* tests: ONE Philox stream consumed in the reference's program order (forces batch = 1 and the
                           general contraction kernel with the reference's list rule): with the generator shim of
                           oracle/ref_rng_shim.c the reference binary then produces the same run, draw for draw */
    const char *resume_read;   /* start from this .resume file if it exists (read_write.F90:384-476; also the file
                                  pypolychord writes for `cube_samples`); NULL = off */
    /* fast/slow parameter grades (chordal_sampling.f90:94-145, generate.F90:303-309): nGrade <= 1 = one grade of nDims
       parameters with num_repeats repeats.  Otherwise grade g owns grade_dims[g] parameters (sum = nDims) and
       grade_repeats[g] directions per chain, drawn in the subspace of its own and all faster parameters;
       num_repeats is then ignored (the total is the sum).  At most 8 grades. */
    int nGrade; const int *grade_dims; const int *grade_repeats;
    int epoch_discard;  /* chains in flight when the list of clusters changes (batch > 1 only).  The reference's farm discards every baby
                           seeded before the change (nested_sampling.F90:313, :339-341: its workers' messages carry positional cluster
                           indices).  0 (default): only the chains seeded in the cluster that ended -- it died or was split -- are lost;
                           the others are samples as good after the change as before and stay in the nursery, their cluster index following
                           the list (BASELINE configs[2] at batch = nlive/2: 199 instead of 338 evaluations per dead point, the reference's
                           linear mode 155).  1: the reference's rule.  Option "epoch_discard" for polychord_c_interface callers. */
    int device_records; /* 1: the run also leaves the records of its points that entered the live set ON THE DEVICE (pchip_result.d_records:
                           what the exchange step of repeat-sharded runs sends; pchip_run_repeats sets it itself).  The dead points of a run
                           are made on the device; without this the merge uploads them again from the host arrays of the result */
    /* sub-dimension clustering (the ini file's `*` parameter marker; settings%sub_clustering_dimensions, nested_sampling.F90:352-367):
       with do_clustering, every update first clusters on these n_sub_cluster cube coordinates, then on all of them.  0-based hypercube
       indices, distances summed in this order (calculate.f90:94-109); an index out of range or given twice fails the run (code 1).
       0 / NULL: plain clustering.  polychord_hip_set_sub_clustering for polychord_c_interface callers. */
    int n_sub_cluster; const int *sub_cluster_dims;
} pchip_settings;

typedef struct {
    int kind;                      /* PCHIP_LIKE_* */
    double mu, sigma;
    const double *invcov;          /* host, row-major D x D (corr gaussian) */
    const double *mean;            /* host, D */
    double logdetcov;
    polychord_loglike_fn fn;       /* callback kind */
    int source;                    /* PCHIP_LIKE_SOURCE: handle from pchip_source_create (ABI 9) */
} pchip_like;

enum { PCHIP_PRIOR_CALLBACK = 0, PCHIP_PRIOR_BOX = 1, PCHIP_PRIOR_TABLE = 2, PCHIP_PRIOR_SOURCE = 3 };
typedef struct {
    int kind;                      /* PCHIP_PRIOR_*: 0 callback, 1 uniform box, 2 table, 3 the source handle's own pchip_prior_param
                                      (pchip_source_create_prior; the handle is pchip_like.source, nothing below is read) */
    const double *lo, *hi;         /* host, D each; NULL => [0,1] */
    polychord_prior_fn fn;
    /* kind == PCHIP_PRIOR_TABLE only (never read otherwise): nDims entries in parameter order, and the hypercube index of every
       parameter (NULL = identity).  With a device likelihood the table is evaluated in the sampling kernels (PCHIP_PATH_DEVICE_PRIOR);
       with a callback likelihood it serves as the host prior.  A table that is a box (all uniform, identity order) runs as kind 1. */
    const pchip_prior_entry *table;
    const int *hyper;
} pchip_prior;

typedef struct {
    double logZ, varlogZ;
    long ndead, nlike, niter, nbatches, nrounds, nupdates;
    int ncluster, ncluster_dead, nTotal, batch;
    double t_generate, t_loop, t_final, t_total;   /* host wall-clock of the phases, seconds */
    double t_setup, t_results, t_teardown;         /* allocation / result download / free */
    double k_time_s[8]; long k_launches[8];        /* HIP-event time per kernel class: nhats, slice, consume, apply,
                                                      clean, covmats, bases drawn ahead on the side stream (profile=1) */
    double *dead, *logweights;     /* [ndead][nTotal] rows [cube|theta|phi|birth|logL], [ndead] */
    double *entry;                 /* [ndead] global contour when the point entered the live set
                                      (== birth column when batch = 1); used by the multi-run merge */
    double *live; int nlive_final; /* live set at termination, before the final kill-off */
    double *logZp, *varlogZp; int nZp;
    double *post_mean, *post_var;  /* [nDims + nDerived] weighted posterior moments of theta, phi */
    long nlike_grade[8];           /* likelihood evaluations per grade (RTI%nlike; the prior samples count for grade 1) */
    int *live_cluster;             /* [nlive_final] 0-based cluster of each row of `live` */
    long nlike_failed;             /* of nlike: evaluations spent on chains whose spawn failed (their last point fell below the
                                      contour that had risen since the nursery was seeded; batch = 1 has almost none) */
    int ncluster_peak;             /* largest number of clusters alive at the same time */
    int epoch_discard;             /* the rule this run followed for chains in flight when the cluster list changed (pchip_settings.epoch_discard:
                                      0 = the engine's, 1 = the reference farm's); it only matters with batch > 1 and several clusters */
    /* settings.device_records: the lived records (logweight > logzero) in death order, in DEVICE memory of device `records_device`, owned
       by the result (pchip_result_free): rows [n_records][nTotal] at d_records, their entry contours at d_records + records_cap * nTotal,
       their own log weights at d_records + records_cap * (nTotal + 1).  NULL when not asked for. */
    double *d_records; long n_records, records_cap; int records_device;
    /* Which kernels the run went through: launches per variant, counted where the host chooses (PCHIP_PATH_* below).  A shape that
       silently leaves a fast path -- an LDS layout that no longer fits, a guard that no longer holds -- shows up here and nowhere
       else: its numbers are the same.  tests/test_baseline_configs.py holds the BASELINE shapes to their paths. */
    long path[24];
} pchip_result;
enum { PCHIP_PATH_CONSUME_PAR = 0,      /* one cluster: the parallel contraction k_consume_par (pc_par.hip) */
       PCHIP_PATH_CONSUME_CL = 1,       /* several clusters: k_consume_clp, decisions in parallel (pc_clus.hip, pc_consume_clp_body.inc) */
       PCHIP_PATH_CONSUME_GENERAL = 2,  /* the general serial kernel k_consume (pc_contract.hip): dynamic nlive, sequential test mode, shapes beyond the LDS */
       PCHIP_PATH_CONSUME_FAST = 3,     /* one cluster, one wavefront: k_consume_fast (B > 1024) */
       PCHIP_PATH_KILLOFF_PAR = 4, PCHIP_PATH_KILLOFF_CL = 5, PCHIP_PATH_KILLOFF_GENERAL = 6, PCHIP_PATH_KILLOFF_FAST = 7,   /* the final kill-off's kernel */
       PCHIP_PATH_UPDATE_FUSED = 8,     /* updates by the fused kernels of pc_update.hip */
       PCHIP_PATH_UPDATE_STEPS = 9,     /* updates by clean + covariance + Cholesky launches (clustered runs, posteriors with boost, nDims beyond the fused kernel) */
       PCHIP_PATH_SLICE_WAVE = 10,      /* nurseries sampled by k_slice (wavefront = chain) */
       PCHIP_PATH_SLICE_LANE = 11,      /* nurseries sampled by k_slice_t (lane = chain: runs in step) */
       PCHIP_PATH_NN_LISTS = 12,        /* candidate-list launches (k_nn_lists) */
       PCHIP_PATH_NN_FALLBACKS = 13,    /* chains whose candidate lists held no living entry: the full search inside the contraction */
       PCHIP_PATH_POOL_MODE = 14,       /* 1: babies written straight into the phantom array */
       PCHIP_PATH_DEFER_UPDATE = 15,    /* 1: the contraction runs past update triggers */
       PCHIP_PATH_CONSUME_CL_SERIAL = 16,   /* several clusters: k_consume_cl, one wavefront deciding chain after chain (settings.ablate bit 10, or an LDS
                                               block the parallel kernel's tables push over the limit) */
       PCHIP_PATH_SUBCLUSTER_PASSES = 17,   /* clustering passes on the sub-clustering coordinates (settings.n_sub_cluster > 0: one per update) */
       PCHIP_PATH_SUBCLUSTER_SPLITS = 18,   /* clusters those passes split */
       PCHIP_PATH_SOURCE_KERNELS = 19,      /* launches of run-time compiled sampling kernels (PCHIP_LIKE_SOURCE, settings.ablate bit 15) */
       PCHIP_PATH_DEVICE_PRIOR = 20,        /* sampling launches (live points, nurseries) that evaluated a prior table or a source prior on the device */
       PCHIP_PATH_SOURCE_TERMS = 21,        /* ... of those of slot 19, the launches whose kernels took the terms form of a source (pchip_source_create_terms) */
       PCHIP_PATH_SLICE_STEP = 22,          /* runs in step: nurseries whose sampling kernel was launched ONCE for several runs (whichever kernel: k_slice_many,
                                               k_slice_t_many); 0 for a run on its own, a group of one, a shape each run launches for itself */
       PCHIP_PATH_DEVICE_BATCH = 23,        /* calls of the device batch callback (polychord_hip_set_device_batch_callback); 0 on every other run */
       PCHIP_PATH_COUNT = 24 };

/* snapshot handed to the update hook: what the reference's file writers see at every update
   (nested_sampling.F90:323-340, read_write.F90) -- host memory owned by the engine, valid during the call */
typedef struct {
    int final_call;                 /* 0: an update; 1: the call after the kill-off (nested_sampling.F90:386-398);
                                       2: the initial live points, before any death (write_prior_file, :197) */
    long ndiscarded;                /* prior samples rejected while the live points were generated */
    long ndead; int nlive, npars;   /* npars = nDims + nDerived + 2 */
    const double *dead;             /* [ndead][npars]  theta, phi, birth contour, logL -- in death order */
    const double *logpost;          /* [ndead] logweight + logL; failed spawns carry logzero + logL */
    const double *live;             /* [nlive][npars], ordered by cluster, then position in the cluster's list */
    const int *live_cluster;        /* [nlive] 0-based cluster of each live row */
    double logZ, logZerr;
    long nlike;
    int ngrade; const long *nlike_grade; const int *grade_dims, *grade_repeats;   /* [ngrade] RTI%nlike / num_repeats per grade */
    int ncluster, ncluster_dead;
    const int *nlive_p;             /* [ncluster] */
    const double *logZp, *logZperr;            /* [ncluster] clusters still active */
    const double *logZp_dead, *logZperr_dead;  /* [ncluster_dead] */
    /* cluster bookkeeping for the per-cluster posterior files (run_time_info.f90:303-505: a split hands every
       child a copy of the parent's posterior points, weights scaled by the evidence fraction it received) */
    const unsigned *dead_cluster;              /* [ndead] id of the cluster each point died in (failed spawns: 0xFFFFFFFF) */
    const unsigned *cluster_uid, *cluster_uid_dead;   /* ids of the active / dead clusters, same order as logZp* */
    int nsplit;                                /* children created by splits so far */
    const unsigned *split_child, *split_parent;
    const double *split_logfrac;               /* log(evidence of child / evidence of parent) at the split */
    /* boost_posterior: phantom points kept as posterior samples (run_time_info.f90:845-870), same row layout */
    int n_extra; const double *extra, *extra_logpost; const unsigned *extra_cluster;
    const unsigned long long *extra_uid;       /* [n_extra] the phantoms' ids (nursery << 32 | chain * num_repeats + baby): what keys their trials */
} pchip_update;
typedef void (*pchip_update_fn)(void *user, const pchip_update *u);

/* optional host hooks of a run */
typedef struct {
    polychord_dumper_fn dumper;   /* called at every update and at the end, like nested_sampling.F90:335,392 */
    pchip_update_fn on_update;    /* same moments; may be NULL */
    void *user;
} pchip_hooks;

/* The structs of this header grow at their END from release to release and carry no size member (their first members are what existing
 * bindings rely on).  A binding that mirrors them (ctypes, ISO_C_BINDING, cgo ...) checks itself against the library it loaded:
 * pchip_abi_version() == PCHIP_ABI_VERSION of the header it was written against, and pchip_sizeof("settings" | "result" | "merged" |
 * "like" | "prior" | "update" | "maximum") == the size of its own mirror (0 for an unknown name). */
/* (still 9 with pchip_prior's two trailing members and PCHIP_PRIOR_TABLE: they are read only when kind == 2, which no earlier caller
 *  sets; pchip_sizeof("prior") tells a mirror of the older layout apart) */
#define PCHIP_ABI_VERSION 9
int  pchip_abi_version(void);
/* A likelihood written as HIP device source, compiled at run time for the device a run is on and evaluated inside the sampling kernels
 * (pchip_like.kind = PCHIP_LIKE_SOURCE, .source = the handle).  The source defines
 *     __device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);
 * a pure, deterministic function; it writes phi[0 .. nDerived) (nDerived <= PCHIP_SOURCE_MAX_DERIVED); a logL at or below logzero marks
 * an invalid point.  `data` (ndata doubles, copied here) is uploaded to the device by every run.  `options`: extra compiler options
 * separated by blanks (-D...), or NULL.  pchip_source_create compiles the user's functions at once: it returns the handle (> 0), or -1
 * with the compiler's log in polychord_hip_last_error().  Needs libhiprtc at run time (dlopen'ed). */
#define PCHIP_SOURCE_MAX_DERIVED 32
int  pchip_source_create(const char *source, const char *options, const double *data, long ndata);
void pchip_source_destroy(int handle);
/* The terms form of a device source, for a likelihood that is a SUM OVER DATA (a chi-square, a fit, a product of per-event densities).
 * Instead of pchip_loglikelihood the source defines
 *     __device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i);
 *     __device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived,
 *                                         const double *data, long ndata);
 * term(i), 0 <= i < nterms, is called by ONE lane of the wavefront per i (lanes take consecutive i: lay records out as a structure of
 * arrays and the loads coalesce); finish gets the finished sum, returns logL and writes all nDerived derived parameters -- cheap, no
 * loop over the data.  The sum has one defined order: lane l adds term(l), term(l + 64), ... in turn to 0.0 (plain IEEE adds of the
 * returned values, never fused with arithmetic inside the term), and the 64 partial sums are added in a balanced pairwise tree over
 * the lanes in lane order ((s0 + s1) + (s2 + s3) ... within rows of sixteen lanes, then (r0 + r1) + (r2 + r3)).  Contract: term is
 * pure, may read theta and data, must not synchronise; finish is pure and must not assume which lane calls it nor that all lanes see
 * the same theta (the derived parameters of a chain's points are written lane = point, from the sum kept when each was accepted: the
 * data are never walked a second time).  One sum per evaluation (several: pchip_source_create_sums).  Same options rule, data block, handle space and
 * pchip_source_destroy as pchip_source_create; nterms >= 1.  pchip_like.kind stays PCHIP_LIKE_SOURCE: the handle knows its form;
 * pchip_result.path[PCHIP_PATH_SOURCE_TERMS] counts the launches that took it. */
int  pchip_source_create_terms(const char *source, const char *options, const double *data, long ndata, long nterms);
/* The terms form with SEVERAL SUMS per evaluation, for a likelihood whose finish needs more than one reduction of the same data (an
 * amplitude or a baseline profiled out analytically: sum m, sum m^2, sum d m; two data sets with a chi-square each; a weighted mean and
 * its variance).  The source defines
 *     __device__ void   pchip_logl_terms(const double *theta, int nDims, const double *data, long ndata, long i, double *t);
 *     __device__ double pchip_logl_finish_sums(const double *sums, const double *theta, double *phi, int nDims, int nDerived,
 *                                              const double *data, long ndata);
 * terms(i), 0 <= i < nterms, is called by ONE lane per i and writes the i-th term of every sum, t[0 .. nsums): one call per (point, i)
 * serves all the sums.  finish_sums gets the finished sums[0 .. nsums), returns logL and writes all nDerived derived parameters -- cheap,
 * no loop over the data.  Each sum k on its own is formed in the order defined for pchip_source_create_terms (lane l adds t_l[k],
 * t_(l + 64)[k], ... to 0.0 by plain IEEE adds, then the balanced tree over the 64 lanes): its bits depend neither on nsums nor on
 * whether the point was evaluated alone or as one end of a bracket.  The contract of term and finish holds for the two functions; an
 * accepted point keeps all its sums, and its derived parameters are finish_sums of them -- the data are never walked a second time.
 * nterms >= 1; 1 <= nsums <= PCHIP_SOURCE_MAX_SUMS (a compile-time constant of the handle's kernels: registers grow with it);
 * with_prior != 0: the source defines pchip_prior_param as well and the handle may run with prior.kind = PCHIP_PRIOR_SOURCE (see
 * pchip_source_create_prior).  Same options rule, data block, handle space, pchip_source_destroy and error reporting as
 * pchip_source_create_terms (-1 with the log in polychord_hip_last_error(); a source that lacks one of its functions fails here, by name);
 * launches count in path[PCHIP_PATH_SOURCE_TERMS] and path[PCHIP_PATH_SOURCE_KERNELS] as a one-sum handle's do. */
#define PCHIP_SOURCE_MAX_SUMS 8
int  pchip_source_create_sums(const char *source, const char *options, const double *data, long ndata, long nterms, int nsums,
                              int with_prior);
/* The QUADRATIC FORM: a Gaussian in data space with a dense covariance, logL = -1/2 r^T P r + const with r = d - m(theta) of length nres
 * and P = C^-1 (binned power spectra, distance ladders, supernova compilations, correlated time series).  The source defines
 *     __device__ double pchip_residual(const double *theta, int nDims, const double *data, long ndata, long i);
 *     __device__ double pchip_logl_finish(double chi2, const double *theta, double *phi, int nDims, int nDerived,
 *                                         const double *data, long ndata);
 * residual(i), 0 <= i < nres, is called by ONE lane per i; finish is the terms form's own, of the finished chi2 = r^T P r, and writes
 * all nDerived derived parameters (an accepted point keeps its chi2: the matrix is never walked a second time).  `precision` is P: host,
 * nres x nres, row-major, copied at creation like the data; it is used EXACTLY as given -- not symmetrised, not factored: chi2 =
 * sum_j r_j sum_i P[i * nres + j] r_i holds for any P.  The user's functions see data / ndata as given.  The defined order:
 *   1. lane l calls residual(i) for i = l, l + 64, ...; the values are kept;
 *   2. for every j:  q_j = 0.0;  for (i = 0; i < nres; ++i) q_j = fma(P[i * nres + j], r_i, q_j)  -- the fused multiply-add of IEEE 754,
 *      rounded once: replay it on the host with fma();
 *   3. t_j = r_j * q_j, one IEEE multiply (not fused with the add that follows);
 *   4. chi2 = the sum of the t_j in the order defined for pchip_source_create_terms: lane l adds t_l, t_(l + 64), ... to 0.0 by plain
 *      IEEE adds, then the balanced tree over the 64 lanes.
 * A point's bits do not depend on whether it was evaluated alone or as one end of a bracket (both ends share ONE walk over P).
 * Contract of residual: pure, may read theta and data, must not synchronise.  To the rest of the library the handle is a terms handle
 * of nres terms and one sum: pchip_like.kind stays PCHIP_LIKE_SOURCE, launches count in path[PCHIP_PATH_SOURCE_TERMS] and
 * path[PCHIP_PATH_SOURCE_KERNELS], pchip_source_eval, pchip_run_in_step and pchip_maximise_device take it as they take any terms handle.
 * 1 <= nres <= PCHIP_SOURCE_MAX_RES (two blocks of residuals, 16 KB of LDS a chain at the limit; P at most 8 MB a run); precision !=
 * NULL; with_prior as for pchip_source_create_sums.  -1 with the reason -- the range, the missing matrix, the compiler's log, the
 * function the source lacks by name -- in polychord_hip_last_error(), before any device call. */
#define PCHIP_SOURCE_MAX_RES 1024
int  pchip_source_create_quad(const char *source, const char *options, const double *data, long ndata, long nres,
                              const double *precision /* host, nres x nres, row-major */, int with_prior);
/* The BATCHED QUADRATIC FORM: the same Gaussian with up to PCHIP_SOURCE_MAX_RES_BATCH residuals (Pantheon+ 1701, DES-SN5YR about 1800, a
 * joint spectrum 2000 - 3000; P is 128 MB a run at the limit), evaluated for MANY points at once on the fp64 matrix cores instead of inside
 * the sampling kernels.  The source defines the two functions of pchip_source_create_quad, pchip_residual and pchip_logl_finish, under the
 * same contract; `precision` is copied behind the data as there and used EXACTLY as given (not symmetrised, not transposed).  A run takes
 * the device batch path (the one behind polychord_hip_set_device_batch_callback) with the library's own evaluator: every round the parked
 * proposals are packed into one block on the device, the box or the prior table is evaluated on the block, and three launches answer it --
 *   1. k_quad_residuals: R[row][i] = residual(theta_row, i), one thread per (row, i), the returned double stored as it is;
 *   2. k_quad_chi2_mm:   Q = R P in 16 x 16 tiles by v_mfma_f64_16x16x4_f64 over i = 0, 4, 8, ...; t_j = Q[row][j] * R[row][j], one IEEE
 *                        multiply; the sixteen t_j of a tile by a fixed butterfly; a wavefront's two tiles in ascending order: one partial
 *                        per row and strip of 32 columns;
 *   3. k_quad_finish:    chi2 = the row's partials added to 0.0 in ascending order, logL = finish(chi2, theta_row, phi, ...), one thread a row.
 * A ROW'S BITS DEPEND ON THAT ROW'S RESIDUALS, ON P AND ON nres ONLY: not on the number of rows, the row's place in the block or the other
 * rows (the split of the columns is a function of nres alone, ragged edges are zero operands, no atomics on doubles).  So pchip_source_eval
 * of a dead point's theta gives the bits the run found, and runs in step (pchip_run_in_step: ONE evaluation a tick for the rows of all
 * runs of a group, one device) are bit for bit their solo runs.  The order is NOT the in-kernel form's: the two agree within their
 * rounding bounds, |chi2 - r^T P r| <= (2 nres + 4) 2^-53 sum_ij |r_i| |P_ij| |r_j| here.
 * Runs: pchip_run / pchip_run_hooks / pchip_run_in_step with like.kind = PCHIP_LIKE_SOURCE under prior.kind 1 (the box) or 2 (a table);
 * a host prior (kind 0) and PCHIP_PRIOR_SOURCE are refused with code 1 and a message before any device call.  path[PCHIP_PATH_DEVICE_BATCH]
 * counts the evaluations, path[PCHIP_PATH_SOURCE_KERNELS] the launches of the two run-time kernels.  Chains per nursery default to
 * nlive / 2 as for a device likelihood.  Not covered: pchip_maximise_device, pchip_run_repeats and pchip_slice_chains refuse the handle
 * with a message; no handle's own prior, no shared values.  1 <= nres <= PCHIP_SOURCE_MAX_RES_BATCH, precision != NULL: -1 with the
 * reason -- the range, the missing matrix, the compiler's log, the function the source lacks by name -- in polychord_hip_last_error(),
 * before any device call.  pchip_source_create_quad is unchanged: its range, its defined fma order and its bits. */
#define PCHIP_SOURCE_MAX_RES_BATCH 4096
int  pchip_source_create_quad_batch(const char *source, const char *options, const double *data, long ndata, long nres,
                                    const double *precision /* host, nres x nres, row-major */);
/* SHARED VALUES: quantities that depend on theta but not on i -- a distance table on a redshift grid that every supernova interpolates,
 * spline coefficients, a model spectrum on a k-grid, rotated parameters, normalisation integrals -- computed ONCE per evaluated point by
 * the wavefront, one lane per value, instead of inside every term.  They go with each of the three wave-parallel forms above.  The source
 * defines one more function,
 *     __device__ double pchip_shared_value(const double *theta, int nDims, const double *data, long ndata, long k);
 * the k-th shared value of the point, 0 <= k < nshared: called by ONE lane per k, once per evaluated point; pure, may read theta and data,
 * must not synchronise, must not read other shared values (a cumulative table is a loop inside it).  The functions of the handle's form are
 * C++ overloads of the names above with one more parameter, `const double *shared`, directly behind theta -- the finished block of
 * nshared doubles:
 *     __device__ double pchip_logl_term   (const double *theta, const double *shared, int nDims, const double *data, long ndata, long i);
 *     __device__ void   pchip_logl_terms  (const double *theta, const double *shared, int nDims, const double *data, long ndata, long i, double *t);
 *     __device__ double pchip_residual    (const double *theta, const double *shared, int nDims, const double *data, long ndata, long i);
 *     __device__ double pchip_logl_finish (double sum_or_chi2, const double *theta, const double *shared, double *phi, int nDims, int nDerived,
 *                                          const double *data, long ndata);
 *     __device__ double pchip_logl_finish_sums(const double *sums, const double *theta, const double *shared, double *phi, int nDims,
 *                                          int nDerived, const double *data, long ndata);
 * Only the overloads of the handle's form are declared and called; the text may carry the others as well.  The form: nres > 0 the quadratic
 * form (precision != NULL, nterms == 0, nsums == 0); otherwise nterms >= 1 with nsums == 0 one sum, with 1 <= nsums <=
 * PCHIP_SOURCE_MAX_SUMS several.  A plain likelihood that wants shared values is nterms = 1.  The defined order:
 *   1. theta goes to the wave's copy in LDS, behind a barrier;
 *   2. lane l calls pchip_shared_value for k = l, l + 64, ... and stores each returned double, untouched, into the point's block; one barrier;
 *   3. the form proceeds exactly as it does without shared values, `shared` pointing at that block: the order of every sum stays what it is.
 * A point's bits do not depend on how it was evaluated: the two ends of a bracket have a block each, filled behind one barrier.  finish
 * receives `shared`, so a derived parameter may be a shared value; an accepted point keeps only its sums, and the block is filled again
 * (step 2) before finish writes its derived parameters.  To the rest of the library the handle is what its form is: path slots,
 * pchip_source_eval, pchip_run_in_step, pchip_maximise_device and the doors take it unchanged.  1 <= nshared <= PCHIP_SOURCE_MAX_SHARED
 * (two blocks of 4 KB of LDS a chain at the limit).  Not provided: values that read each other, shared values for pchip_loglikelihood's
 * own entry point or for pchip_prior_param, values kept across the points of a chain.  -1 with the reason -- the range, the missing
 * matrix, the mixed form, the compiler's log, the function the source lacks by name -- in polychord_hip_last_error(), before any device
 * call. */
#define PCHIP_SOURCE_MAX_SHARED 512
int  pchip_source_create_shared(const char *source, const char *options, const double *data, long ndata,
                                long nshared, long nterms, int nsums, long nres, const double *precision, int with_prior);
/* The user's PRIOR in the same source and the same handle as the likelihood (pchip_prior.kind = PCHIP_PRIOR_SOURCE with pchip_like.kind =
 * PCHIP_LIKE_SOURCE, .source = the handle).  Besides the likelihood functions of its form -- nterms == 0: pchip_loglikelihood; nterms
 * >= 1: pchip_logl_term and pchip_logl_finish -- the source defines
 *     __device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata);
 * which returns theta[i].  It is called once per parameter, lane = parameter: `cube` is the whole hypercube point (nDims doubles,
 * read-only, hypercube order = parameter order; the source may read any coordinate, so a dependent prior -- a Cholesky factor, a
 * hyper-parameter, an ordered block -- loops in its lane), `data` the handle's data block, the one the likelihood sees.  Contract: pure,
 * deterministic, must not synchronise; only ever called for points inside the unit cube; the likelihood receives exactly the values
 * returned.  Same options rule, data block, handle space and pchip_source_destroy as pchip_source_create; a source that lacks one of
 * its functions fails here, by name.  The handle also runs under prior.kind 1 and 2, as one without a prior does.  A prior source for a
 * built-in or callback likelihood (a prior-only handle) and pchip_run_repeats are not supported: the run fails with a message (several
 * seeds in step: pchip_run_in_step).  At the PolyChord-interface doors: polychord_hip_set_source, then polychord_hip_source_loglike and
 * polychord_hip_source_prior as the callbacks (Part 2's first block).  Launches are counted in path[PCHIP_PATH_DEVICE_PRIOR] and path[PCHIP_PATH_SOURCE_KERNELS]. */
int  pchip_source_create_prior(const char *source, const char *options, const double *data, long ndata, long nterms);
/* The prior of such a handle at n hypercube points, cubes[n][nDims] -> thetas[n][nDims] (host arrays): one wavefront a point, through
 * the transform code of the sampling kernels.  Return codes as pchip_source_eval. */
int  pchip_source_prior_eval(int handle, const double *cubes, long n, int nDims, double *thetas);
/* A source likelihood (either form) at n points, thetas[n][nDims] -> logL[n], phi[n][nDerived] (host arrays; phi may be NULL when
 * nDerived is 0): one wavefront a point, through the evaluation code of the sampling kernels.  For tests, and for users checking their
 * source against a host version.  (A batched quadratic form, pchip_source_create_quad_batch: the three launches of its runs for all n
 * rows, the same bits as inside a run.)  0, or 1 with a message in polychord_hip_last_error(), 2 no device / HIP error, 3 nDims > 256. */
int  pchip_source_eval(int handle, const double *thetas, long n, int nDims, int nDerived, double *logL, double *phi);
unsigned long pchip_sizeof(const char *struct_name);
void pchip_settings_default(pchip_settings *s, int nDims, int nDerived);
int  pchip_device_count(void);
/* full run; returns 0 on success, else (message on stderr, nothing to free, the process goes on): 1 settings, 2 HIP /
   device error, 3 nDims unsupported, 4 a working set beyond the LDS, 5 stopped on request, 6 resume file, 7 out of
   memory, 8 a capacity limit */
int  pchip_run(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, pchip_result *out);
int  pchip_run_hooks(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior,
                     const pchip_hooks *hooks, pchip_result *out);
void pchip_result_free(pchip_result *r);
/* `maximise = T` (maximiser.F90:32-224, nelder_mead.f90, write_max_file read_write.F90:754-807): Nelder-Mead polish of
   the best live points of a finished run into the maximum-likelihood and maximum-posterior points, written to `path`
   (<base_dir>/<file_root>.maximum).  Host code; live rows as in pchip_result.  0 on success. */
int  pchip_maximise(polychord_loglike_fn loglikelihood, polychord_prior_fn prior, int nDims, int nDerived, double logzero,
                    const double *live, const int *live_cluster, int nlive, const double *post_mean, const char *path);
/* The maximiser's result as values, and the maximiser for problems that live wholly on the DEVICE (a built-in or a source likelihood of either
 * form under the uniform box, a prior table or the handle's own source prior: nothing that has a host function to polish through).
 * Index [0] is the likelihood leg, [1] the posterior leg: status 0, or 1 "Could not construct simplex" (no cluster of the live set holds
 * nDims + 1 rows above logzero: nothing is searched and nothing launched for that leg); cluster = the cluster the simplex came from;
 * niter = Nelder-Mead iterations that moved the simplex, neval = likelihood calls of the search (a trial point outside the unit cube is
 * logzero without one, calculate.f90:36-38).  A run whose likelihood leg has no simplex stops there: its posterior leg is status 1, cluster -1.
 * Points are [theta | phi]; max_post = logl_at_post + dXdtheta(post point); mean_point = [mean theta | phi at the mean theta], as
 * loglikelihood(mean) leaves it (maximiser.F90:77-80).  The point arrays are owned by the struct (pchip_maximum_free); a zeroed struct is a
 * valid empty one, and every door that takes an `out` leaves each struct zeroed or filled on every return, refusals included, so
 * pchip_maximum_free may follow unconditionally. */
typedef struct { int status[2], cluster[2]; long niter[2], neval[2];     /* [0] likelihood leg, [1] posterior leg */
                 double max_logl, *max_point;                              /* [nDims + nDerived] */
                 double max_post, logl_at_post, *post_point;
                 int has_mean; double logl_mean, *mean_point; } pchip_maximum;
/* pchip_maximise without its file: the host path (host function pointers), the same searches in the same order.  0, or 1 when a leg has no
 * simplex (status[] tells which). */
int  pchip_maximise_values(polychord_loglike_fn loglikelihood, polychord_prior_fn prior, int nDims, int nDerived, double logzero,
                           const double *live, const int *live_cluster, int nlive, const double *post_mean, pchip_maximum *out);
/* The device maximiser: one wavefront per problem (a run's likelihood leg, its posterior leg), the simplex in LDS, the evaluation code of the
 * sampling kernels (the bits of pchip_source_eval / pchip_prior_transform), nelder_mead.f90's rules with dl = 1e-5 and at most max_iter
 * iterations (<= 0: 200000, the host's cap).  Of `s` nDims, nDerived, logzero, device and ablate are read; live rows as in pchip_result.
 * nDims <= 64.  0; 1 with a message in polychord_hip_last_error() (a callback likelihood or a callback prior is refused before any device call;
 * a leg without a simplex: status[], the other values stay); 2 no device / HIP error; 3 nDims > 64 (the host maximiser remains for host functions). */
int  pchip_maximise_device(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, const double *live, const int *live_cluster,
                           int nlive, const double *post_mean, long max_iter, pchip_maximum *out);
/* ... for the final live sets of nruns runs of one problem (pchip_run_in_step's results): two launches for all runs -- the candidate values
 * of every posterior leg, then every leg of every run.  out[r] is bit for bit pchip_maximise_device of run r alone. */
int  pchip_maximise_device_many(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nruns, const pchip_result *runs,
                                long max_iter, pchip_maximum *out /* [nruns] */);
/* <root>.maximum of a pchip_maximum (write_max_file, read_write.F90:754-807): what pchip_maximise writes.  0; 1 a leg has no result; 2 the file */
int  pchip_maximum_write(const pchip_maximum *m, int nDims, int nDerived, const char *path);
void pchip_maximum_free(pchip_maximum *m);
/* ---- repeat-sharded runs: independent runs of one problem, merged ------------------------------------
 * The reference's way to use more hardware is its MPI farm (nested_sampling.F90:262-301, mpi_utils.F90:376-463: workers'
 * babies gathered into one run).  Here every GPU carries a complete run of its own; the dead points of all runs are
 * gathered and their union -- a nested-sampling run with n(L) = sum of the runs' live points -- gives one evidence
 * (error ~ 1/sqrt(runs)) and one posterior. */
typedef struct {
    double logZ, varlogZ;          /* evidence of the union (log-normal location and variance, run_time_info.f90:652-678) */
    long n; int nTotal, nruns;     /* points that entered a live set, over all runs */
    double *rows;                  /* [n][nTotal] merged dead points ascending in logL (host; only if asked for); the birth
                                      column holds the contour at which the point ENTERED its live set */
    double *logweights;            /* [n] log prior-volume weight logX_i - log(n_i + 1) of each merged point */
    int *nlive;                    /* [n] live points over all runs just before each death */
    double *post_mean, *post_var;  /* [nDims + nDerived] posterior moments of theta, phi */
    double t_merge_s, t_runs_s;    /* wall clock of the merge / of the runs (pchip_run_repeats) */
    long nlike, ndead_all;         /* totals over the runs (pchip_run_repeats) */
    double runs_logZ_mean, runs_logZ_sem;   /* mean of the runs' OWN log Z and its standard error (one run: that run's own error) */
    /* Which evidence `logZ, varlogZ` (and `logweights`, `post_mean`, `post_var`) are: evidence_rule
     *   0 -- no run ever held more than ONE cluster: the replay of the union from ranks and live counts (the sharper estimator, and what
     *        anesthetic computes from <root>_dead-birth.txt); logZ_replay == logZ;
     *   1 -- at least one run held several clusters at some time (pchip_result.ncluster_peak > 1; `nclustered` of them).  Such a run weighs a dead point by
     *        its CLUSTER's volume over the cluster's live count (run_time_info.f90:211-296, volumes apportioned at a split :458-503), which
     *        the replay does not know (10-D Rastrigin, dozens of clusters: the replay sits 0.46 below the runs' own log Z, twenty of its own
     *        error bars).  Then logZ, varlogZ = the runs' own evidences combined in linear space -- log-normal moments of each run,
     *        mean of the Z_r, variance the larger of the propagated one and the scatter between the runs -- and record i of a run keeps its
     *        OWN log weight minus log(nruns): sum_i w_i L_i over the union = the mean of the runs' Z_r, so the union's posterior is the
     *        Z_r-WEIGHTED mixture of the runs' posteriors (run r carries Z_r / sum Z), not an equal-weight one.  The replay stays in
     *        logZ_replay, varlogZ_replay; `nlive` is the replay's live count either way -- and <root>_dead-birth.txt of such a union, read
     *        by anesthetic, reproduces logZ_replay, not the log Z written in <root>.stats. */
    double logZ_replay, varlogZ_replay;
    int evidence_rule, nclustered;
} pchip_merged;
/* Merge `nruns` runs on the device.  rows = the lived records (logweight > logzero) of run 0, then run 1, ...: counts[q]
 * rows of nTotal doubles each, every run ascending in logL (the order in which they died); entry[i] = contour at which
 * record i entered its live set (pchip_result.entry).  on_device: the two arrays are device pointers (e.g. the buffer an
 * RCCL all-gather filled), else host memory that is uploaded first.  Returns 0, or a pchip_run code; no CPU path. */
int  pchip_merge_records(int nDims, int nDerived, int nruns, const long *counts, const double *rows, const double *entry,
                         int on_device, int want_rows, pchip_merged *out);
/* The same with what each run knows about itself: ownw[i] = the log prior-volume weight record i had in its own run
 * (pchip_result.logweights of the lived records, laid out like `entry`), run_logZ / run_varlogZ / run_clustered[q] = the run's own
 * evidence and whether it ever held more than one cluster (pchip_result.ncluster_peak > 1).  If any run did, the union's evidence and
 * weights follow pchip_merged.evidence_rule 1; all four NULL = pchip_merge_records. */
int  pchip_merge_records_ex(int nDims, int nDerived, int nruns, const long *counts, const double *rows, const double *entry,
                            const double *ownw, const double *run_logZ, const double *run_varlogZ, const int *run_clustered,
                            int on_device, int want_rows, pchip_merged *out);
void pchip_merged_free(pchip_merged *m);
/* <root>.stats (global evidence, counters, posterior means), <root>_dead-birth.txt and <root>.txt of a merged result in
 * the reference's formats (read_write.F90:809-910, :707-716, :479-617), so that PolyChordOutput / anesthetic read the
 * union like a single run.  0 on success. */
int  pchip_merged_write(const pchip_merged *m, int nDims, int nDerived, const char *base_dir, const char *file_root);
/* nseeds independent runs (settings `s` with seed = seeds[k]) spread over `devices` (ordinals of this process; NULL / 0 =
 * the device of `s`), at most max_in_flight at a time per device, one host thread each; results[k] as from pchip_run
 * (free each with pchip_result_free), merged (may be NULL) = their union with rows.  0 on success. */
int  pchip_run_repeats(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nseeds, const int *seeds,
                       int ndevices, const int *devices, int max_in_flight, pchip_result *results, pchip_merged *merged);
/* the same; want_rows = 0: the union without its merged rows (evidence, weights, live counts, moments only: 370 MB less to bring back
   for sixteen runs of the metric configuration) */
int  pchip_run_repeats_ex(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nseeds, const int *seeds,
                          int ndevices, const int *devices, int max_in_flight, int want_rows, pchip_result *results, pchip_merged *merged);
/* The runs in step for any problem that is wholly on the device: a built-in or a source likelihood (plain or terms form), under the uniform
 * box, a prior table or the handle's own source prior (prior.kind 1, 2, 3), and settings.ablate bit 15.  Arguments, results, merge and
 * return codes of pchip_run_repeats_ex; the seeds are dealt to the devices and their scheduler groups in the same way, up to max_in_flight
 * runs of a device go round by round together, and every kernel of a round is launched once for all of them.  Every run is bit for bit
 * pchip_run of its seed.  path[PCHIP_PATH_SLICE_STEP] counts a run's nurseries whose sampling launch was shared; a shape without a shared
 * launch (nDims > 64 behind the bases kernels, parameter grades, the sequential stream, the correlated Gaussian) still goes round by round
 * with the others and launches its own k_slice.  A host callback likelihood or a host prior (kind 0) is refused with code 1 and a message,
 * before any device call; prior.kind 3 with a handle that defines no prior fails as pchip_run does.  (pchip_run_repeats keeps refusing a
 * source handle and runs a table one thread per run.)
 * A callback likelihood (like.kind == PCHIP_LIKE_CALLBACK, like.fn not NULL) is taken while a DEVICE batch callback is registered at the time
 * of the call (polychord_hip_set_device_batch_callback, which has the contract): the runs of a group tick together, their parked proposals
 * are packed into one block, and the caller's function is called once a tick for all of them, on the calling thread.  One device (ndevices
 * > 1 is refused with code 1 and a message) and one group at a time, without scheduler threads whatever do_clustering says.  prior.kind 1 / 2:
 * the engine's transform on the whole block (flags bit 0); prior.kind 0: the callee makes the prior itself (flags 0) -- no host prior function
 * is called by a run in step; prior.kind 3 is refused.  The live points are made run by run during set-up (nprior rows a call).
 * path[PCHIP_PATH_DEVICE_BATCH] of a run counts the calls that carried rows of that run: the solo run's count. */
int  pchip_run_in_step(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nseeds, const int *seeds,
                       int ndevices, const int *devices, int max_in_flight, int want_rows, pchip_result *results, pchip_merged *merged);

/* ---- between processes: one rank per GPU, RCCL inside the library (dlopen of librccl.so at first use, none at link time).
 * Replaces the reference's MPI exchange (mpi_utils.F90:376-463 throw_baby / catch_babies, nested_sampling.F90:262-301) for
 * the repeat-sharded mode: the only message of a job is ONE all-gather of the runs' lived records at its end.
 *   pchip_comm_get_id: 128 opaque bytes (an ncclUniqueId) made by ONE rank and handed to all others by the caller -- a
 *       file, MPI_Bcast, a torch.distributed store: the library does not care;
 *   pchip_comm_create: collective over the nranks processes (ncclCommInitRank), `device` = this rank's HIP ordinal;
 *   pchip_comm_merge: picks the points of `run` that entered a live set (logweight > logzero) on the device, all-gathers
 *       the counts and then one padded block [nmax][nTotal] | [nmax] | [nmax] per rank (ncclAllGather over xGMI), and merges the
 *       union on every rank with pchip_merge_records; nlike / ndead_all of the result are the totals over the ranks.
 *       c = NULL: this process alone (no collective library is touched).
 * All return 0 or a pchip_run code; nothing has a CPU path. */
typedef struct pchip_comm pchip_comm;
#define PCHIP_COMM_ID_BYTES 128
int  pchip_comm_get_id(char *id128);
int  pchip_comm_create(const char *id128, int nranks, int rank, int device, pchip_comm **out);
void pchip_comm_destroy(pchip_comm *c);
int  pchip_comm_merge(pchip_comm *c, const pchip_result *run, double logzero, int nDims, int nDerived, int want_rows,
                      pchip_merged *out);
/* the same for a rank that holds `nruns` runs (pchip_run_repeats with merged = NULL: the runs of a GPU in step): the ranks' run
 * counts travel first, then six words per run (count, nlike, ndead, log Z, var log Z, clustered?), then ONE padded block per rank
 * [nmax][nTotal] | entry [nmax] | own log weight [nmax] with the rank's runs one after the other; the union of all ranks' runs is
 * merged on every rank (pchip_merge_records_ex).  Ranks may hold different numbers of runs. */
int  pchip_comm_merge_many(pchip_comm *c, const pchip_result *runs, int nruns, double logzero, int nDims, int nDerived, int want_rows,
                           pchip_merged *out);
/* The same exchange over the CALLER's collective instead of RCCL: all_gather(user, send, recv, bytes) places every rank's `bytes` at `send`
 * (device memory of `device`) into `recv` (device memory, nranks * bytes, rank after rank) on all ranks; it is called with the library's stream
 * drained and returns 0 once `recv` is complete.  For a host that brings its own transport (a GPU-aware MPI_Allgather under the reference's
 * MPI launcher, mpi_utils.F90:376-463; torch.distributed) and for tests with several ranks on one GPU, where RCCL forms no communicator.
 * pchip_comm_merge / _merge_many / _destroy take the communicator like one made by pchip_comm_create. */
typedef int (*pchip_allgather_fn)(void *user, const void *send, void *recv, unsigned long bytes);
int  pchip_comm_create_with(pchip_allgather_fn all_gather, void *user, int nranks, int rank, int device, pchip_comm **out);
const char *pchip_comm_library(void);   /* the RCCL that was resolved (path or soname), NULL if none could be loaded */

/* kernel-level: directions + slice chains only (parity tests against oracle pc_slice_chain) */
int  pchip_slice_chains(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior,
                        unsigned batch, int nchains, const double *seeds, const double *chol,
                        double contour, double *babies_out, double *nhats_out, int *nlike_out);
/* kernel-level: the directions alone (Gaussian deviates, Gram-Schmidt, whitening with the Cholesky factor) by the launcher a run takes --
 * accuracy tests against a long double reference (tests/test_directions.py).  Set up as pchip_slice_chains: one cluster, chain c seeded
 * from seeds[c] (a row of nTotal doubles), chol [nDims][nDims] for all chains; no slice is sampled.
 * path 0 = the whole kernels (what pchip_slice_chains launches); path 1 = the split launch of a run on its own, bases first, then seeds and
 * whitening; path 2 = path 1 with the packed bases (one grade, nDims 2 ... 24).  A path that the state does not have (a shape that does
 * not split, nDims > 256) returns PCHIP_NO_SUCH_PATH and launches nothing.
 * Out (host memory): nhat [nchains][num_repeats][nDims] in generation order (not shuffled), nhat_w [nchains][num_repeats]; where the run
 * would form them (correlated Gaussian, 64 < nDims <= 128: *has_Ms = 1) nhat_Ms [nchains][num_repeats][nDims] and ch_My [nchains][nDims]
 * (either may be NULL); on paths 1 and 2 raw [nchains][bases][nDims][nDims], the orthonormal bases before whitening, basis after basis
 * over all grades, vector after vector (of a grade that starts at parameter `off`, nDims - off vectors are written).  nrows, nbases: the
 * directions per chain and the bases per chain that the caller's arrays were sized for; if the settings give other numbers: 1.
 * 0, 1 (bad arguments, message in polychord_hip_last_error()), PCHIP_NO_SUCH_PATH, else a pchip_run code. */
#define PCHIP_NO_SUCH_PATH 64
int  pchip_directions(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, unsigned batch, int nchains,
                      const double *seeds, const double *chol, int path, double *nhat_out, double *nhat_w_out,
                      double *nhat_Ms_out, double *ch_My_out, int *has_Ms, double *raw_out, int nrows, int nbases);
/* kernel-level: the deck records that the first half of the split launch leaves behind the bases of a nursery (nDims <= 24, one grade, keyed
 * draws, num_repeats <= 64): per chain 66 ints, [tag low word, tag high word, deck[64]] -- deck[p] is the direction slice p of the chain
 * takes (the first stays, the others are shuffled), the tag a function of (seed keys, batch, chain, num_repeats) under which the sampling
 * kernel recognises the record.  Set up as pchip_directions, bases only, by the kernel a run on its own takes (settings.ablate bit 19: the
 * kernel with a wavefront a basis).  records [nchains][66] (host memory) is IN and OUT: it is placed behind the bases before the launch, so
 * where no record is written (num_repeats > 64) it comes back as it was.
 * 0, 1 (bad arguments, message in polychord_hip_last_error()), PCHIP_NO_SUCH_PATH (nDims > 24, grades, the sequential stream), else a
 * pchip_run code. */
int  pchip_deck_records(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, unsigned batch, int nchains, int *records);
/* kernel-level: the DEVICE transform of a prior table(prior->kind == PCHIP_PRIOR_TABLE) at n hypercube points, cube [n][nDims] in,
 * theta [n][nDims] out (host memory) -- parity tests against polychord_hip_table_prior.  0, 1 (a bad table, message in
 * polychord_hip_last_error()), 2 (no device), 3 (nDims > 256). */
int  pchip_prior_transform(const pchip_prior *prior, int nDims, int n, const double *cube, double *theta, int device);
/* kernel-level: the covariance and the Cholesky factor an update makes (calculate_covmats + calc_cholesky behind clean_phantoms) of given
 * rows, by the run's own launchers -- accuracy tests against a long double reference (tests/test_update_factors.py).  Of `s` nDims,
 * ablate and device are read.  Host arrays in: live [nlive][nDims] cube coordinates with a 0-based cluster per row; phantom
 * [nph][nDims] with a logL and a cluster per row, cluster -1 = the row holds no phantom; threshold [ncluster]: a phantom counts unless
 * logL < threshold of its cluster; shift [nDims] or NULL (the cube centre).  path 1 = the fused update (one cluster, nDims <= 128,
 * nph >= 1; settings.ablate bits 1 and 16 choose compacting mode and the chain), path 0 = the general steps (clean, covmats).
 * Out: cov, chol [ncluster][nDims][nDims]; count [ncluster], the rows that were counted; shift_out [nDims] (may be NULL), the next
 * update's shift (path 0: the shift as given); *chol_suspect (may be NULL), PcCtl::chol_suspect after the update.
 * 0, 1 (bad arguments, message in polychord_hip_last_error()), 2 (no device), 3 (nDims > 256), else a pchip_run code. */
int  pchip_update_factors(const pchip_settings *s, int ncluster, int nlive, const double *live, const int *live_cluster,
                          int nph, const double *phantom, const double *ph_logL, const int *ph_cluster, const double *threshold,
                          const double *shift, int path, double *cov, double *chol, int *count, double *shift_out, int *chol_suspect);
/* kernel-level: the clustering of an update (do_clustering + add_cluster, the kNN kernels of pc_cluster.hip and the host's recursion) on
 * given point sets, by the run's own launchers -- tests against the reference's answers on ties, duplicates and tile edges
 * (tests/test_clustering_kernels.py).  Of a set's settings nDims, device, ablate, n_sub_cluster and sub_cluster_dims are read.
 * In, per set: ncluster clusters; nlive live slots, slot i with cube coordinates live[i][nDims], live_logL[i] and live_cluster[i] (0-based;
 * -1: the slot is dead) -- a point's list position is its rank among the rows of its cluster; nph phantom rows with cube coordinates, logL
 * and cluster (-1: the row holds no phantom).  The clusters get the ids 0 ... ncluster - 1 and fixed distinct volumes and evidences,
 * logXp[c] = log((c + 1) / sum) among them; out->init hands them back.
 * path 0 (one set): the state is installed as a run holds it at the start of an update and ClusterUpdate::do_clustering is called as
 * Engine::do_update calls it (with sub-dimensions: the sub pass, then the full pass) -- the one-run launchers.
 * Out, per set (host memory, sized by the caller: maxc clusters, nsplit_cap genealogy entries; every pointer but the scratch is needed):
 * the state after the update.  cl_list holds the clusters' slots one cluster behind the other in list order (cl_n[c] each).  ph_cluster is
 * the phantoms' cluster index (-1: gone); ph_count k_ph_count's counts of the last split (-1 each if nothing split).  XpXq has the leading
 * dimension maxc.  init: [5][ncluster] logXp, logZp, logZXp, logZp2, logZpXp as installed, then XpXq [ncluster][ncluster].
 * scratch_Sm / scratch_knn [scratch_cap^2] and scratch_lab [scratch_cap], all three or none: the first pass's similarity block, neighbour
 * lists and first-level labels (1-based) of the first cluster the pass looks at, scratch_n its points (with sub-dimensions: of the sub pass).
 * path 1 (nsets >= 1 sets at once, which may differ in size, in clusters and in sub-dimensions): the launchers of the runs in step -- the first
 * pass of all sets in one launch, every level of their recursions in one launch each, from records laid down by the cohort's own code; one
 * pass per set (a set with sub-dimensions: its sub pass), and no split is made.  Out: live_cluster as given, live_pos[i] the part (1-based,
 * numbered by first appearance in list order) of slot i within its cluster, cl_n[c] the parts of cluster c, ncluster as given, levels, and
 * the scratch where asked for; the other arrays are not written.
 * A path that does not exist: PCHIP_NO_SUCH_PATH, nothing launched.
 * 0, 1 (bad arguments, message in polychord_hip_last_error()), PCHIP_NO_SUCH_PATH, else a pchip_run code (4: a cluster too large for the
 * LDS kNN sort -- nothing of the clustering is launched then). */
typedef struct {
    int ncluster, nlive, nph;
    const double *live, *live_logL; const int *live_cluster;
    const double *phantom, *ph_logL; const int *ph_cluster;
} pchip_cluster_in;
typedef struct {
    int maxc, nsplit_cap, scratch_cap;                     /* in: what the arrays below have room for */
    int ncluster, nsplit, levels, scratch_n;               /* out: clusters after the update, genealogy entries, levels of the recursion launched */
    int *live_cluster, *live_pos, *cl_list;                /* [nlive] */
    int *cl_n, *imin_slot, *ph_count; unsigned *cl_uid;    /* [maxc] */
    double *logLp, *lse_ref, *lse_sum, *logXp, *logZp, *logZXp, *logZp2, *logZpXp;      /* [maxc] */
    double *XpXq;                                          /* [maxc][maxc] */
    int *ph_cluster;                                       /* [nph] */
    unsigned *split_child, *split_parent; double *split_logfrac;      /* [nsplit_cap] */
    double *init;                                          /* [5 * ncluster + ncluster^2] */
    double *scratch_Sm; int *scratch_knn, *scratch_lab;    /* optional */
} pchip_cluster_out;
int  pchip_cluster_update(const pchip_settings *s, int nsets, const pchip_cluster_in *in, pchip_cluster_out *out, int path);

/* The pack of the device batch callback alone (tests/test_park_pack.py), host arrays in and out, the product's two kernels in between:
 * need [nchains] (a chain waits for an answer: non-zero), prop [nchains][nDims]  ->  rank [nchains] (the ascending enumeration of the chains
 * with need, -1 for the others), *count, and cube [>= count][nDims]: row rank[c] = prop[c].  Rows of `cube` from count on are not written.
 * 0, or 1 (arguments) / 2 (device). */
int  pchip_park_pack(int nchains, int nDims, const int *need, const double *prop, int *rank, int *count, double *cube, int device);
/* ... of a group of 1 <= nruns <= 64 runs in step (tests/test_park_pack_many.py): run r has nchains[r] >= 1 chains; need, prop and rank hold
 * the runs one behind the other.  rank: the row in the ONE block -- the counts of the runs before + the run's own ascending enumeration, -1
 * without need --, counts [nruns], *total, and cube [>= total][nDims]; rows of `cube` from the total on are not written.  0, 1 or 2 as above. */
int  pchip_park_pack_many(int nruns, const int *nchains, int nDims, const int *need, const double *prop, int *rank, int *counts, int *total,
                          double *cube, int device);

/* The acceptance of the one-cluster parallel contraction alone (tests/test_par_accept.py), host arrays in and out, the contraction's own
 * device functions for its binary search, ranks and acceptance in between, one workgroup of 1024 threads on the keys of the logL given:
 * snapshot_logL [n] ascending (1 <= n <= 8192), cand_logL [T] by step (1 <= T <= 1024), valid [T] (non-zero: a step of the current epoch)
 * ->  accept [T] (1: the candidate of step t replaces the lowest live point).  serial != 0: by the serial recurrence (settings.ablate bit 18).
 * 0, or 1 (arguments) / 2 (device). */
int  pchip_par_accept(int n, const double *snapshot_logL, int T, const double *cand_logL, const unsigned char *valid, int serial,
                      unsigned char *accept, int device);

#ifdef __cplusplus
}
#endif
#endif
