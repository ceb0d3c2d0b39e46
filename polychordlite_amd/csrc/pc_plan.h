// pc_plan.h -- which kernels a run, a nursery, a contraction and an update take: the host loop's policy, in one place.
//
// Host only: plain structs and pure functions, no HIP call.  Included by pc_engine.hip (and by tools/dev/plan_record.hip, which walks every
// function below over the full grid of its facts and compares the answers with the conditions of the commit before this header existed,
// ba2108c: tests/test_run_plan.py).  It does not see Engine.  What a launcher's own predicate says (pc_par_fits, pc_fast_fits,
// pc_consume_cl_fits, pc_consume_clp_fits, pc_update_fused_ok, pc_slice_t_ok, pc_bases_t_ok, pc_slice_fusable, pc_nhats_splittable) comes in
// as a boolean: the engine asks each of them at ONE place (Engine::make_plan, nursery_facts, contract_facts, update_facts).
//
// A decision is three things, and a new one is added by adding the three:
//   its facts       what is known at the moment it is made (Pc*Facts)
//   its choice      pc_choose_*(plan, facts): an enumerator -- the comment at the enumerator says WHY the branch exists -- and what goes with it
//   its counters    pc_count(path, choice): the pchip_result.path[] slots the choice adds to.  The engine counts nowhere else, except what the
//                   device reports or a launcher's return value decides (the kill-off, the candidate lists' fallbacks, the sub-clustering passes)
// The engine switches over the choice and does the mechanics: streams, events, stage() / co->rec(), cursors.
#pragma once
#include "pc_state.h"
#include "polychord_hip.h"
#include <cstdlib>
#include <algorithm>

// ---- developer switches of the environment that pc_engine.hip reads (A/B of one code path against another on the same box; production sets
//      none: tools/dev/README.md).  Read once, on first use.  The switches of the launchers stay with the launchers.
struct PcEnv {
    static bool set(const char *n) { return std::getenv(n) != nullptr; }
    static bool zero(const char *n) { const char *e = std::getenv(n); return e && std::atoi(e) == 0; }      // VAR=0 switches a default off
    static int num(const char *n, int dflt) { const char *e = std::getenv(n); return e ? std::atoi(e) : dflt; }
    const int debug = num("PC_DEBUG", 0);                                   // 2-5: cycle counters and phase times on stderr
    const bool poison = set("PC_POISON");                                   // fresh device blocks are filled with 0x5A bytes
    const bool side_pick_off = set("PC_SIDE_PICK_OFF");                     // a side stream from the pool as it comes, its hardware queue not looked at
    const bool ms_pre_off = set("PC_MS_PRE_OFF");                           // correlated Gaussian, nDims > 64: M.n^ inside k_slice, not by the bases' kernel
    const bool nhats_split_off = set("PC_NHATS_SPLIT_OFF");                 // no buffers for the split launch of the bases: the whole kernel
    const int raw_depth = std::max(2, num("PC_RAW_DEPTH", 3));              // ring of bases buffers (the engine caps it at its ring)
    const bool copy_batch_off = set("PC_COPY_BATCH_OFF");                   // an update's small copies as hipMemcpyAsync calls, not one k_copy_batch
    const bool notify_off = set("PC_NOTIFY_OFF");                           // the round's outcome by copy + wait, not by the stamped host mirror
    const bool presort_off = set("PC_PRESORT_OFF");                         // clustered run on its own: k_sort_live in line, not beside k_slice
    const bool side_free = set("PC_SIDE_FREE"), side_ordered = set("PC_SIDE_ORDERED");      // the side stream's bases beside / behind k_slice whatever nDims
    const bool nn_lists_off = set("PC_NN_LISTS_OFF");                       // no candidate lists: every launch of a clustered run by the general kernel
    const bool cohort_general_off = zero("PC_COHORT_GENERAL");              // runs in step: only the lane = chain kernels are launched for all at once
    const bool cohort_final_aside_off = zero("PC_COHORT_FINAL_ASIDE");      // ... a clustered run's kill-off on the common stream
    const bool cohort_side_off = zero("PC_COHORT_SIDE");                    // ... no second stream for the next nursery's bases
    const bool cohort_copy_streams_off = zero("PC_COHORT_COPY_STREAMS");    // ... a copy stream per run
    const bool cohort_fibers_off = zero("PC_COHORT_FIBERS");                // ... a run's waits are its own, not shared through fibers
    const int cohort_setup_threads = std::max(1, num("PC_COHORT_SETUP_THREADS", 1));      // ... threads that set the runs up
};
inline const PcEnv &pc_env() { static const PcEnv e; return e; }

// ---- a run ----------------------------------------------------------------------------------------------------------------------------
struct PcRunFacts {
    int ablate, force_general;
    bool fixed_nlive;                   // no dynamic-nlive table, nprior >= nlive, a resumed run with its nlive points
    bool par_fits, fast_fits;           // pc_par_fits, pc_fast_fits
    bool fused_fits_one;                // pc_update_fused_ok for one cluster
    bool clustering, boost;             // do_clustering; boost_posterior != 0
    bool dumper, on_update, resume_write;
    bool seq_mode, posteriors;          // sequential-stream test mode; posteriors || equals
    bool callback;                      // the host evaluates the likelihood
};
enum PcCtlRead { PC_CTL_NONE = 0,       // nobody on the host looks at evidences, counters or cluster ids at an update
                 PC_CTL_EARLY,          // read in front of the update: the hooks and files see the block before the clean
                 PC_CTL_LATE };         // clustering alone: the block comes with the counts, in the same wait
struct PcRunPlan {
    int ablate; bool seq_mode;
    // the one-cluster kernels assume a static number of live points; each has its own LDS budget
    bool static_ok, par_ok, fast_ok;
    bool cl_ok;                         // several clusters: the one-wave contraction may be taken (static, force_general == 0, not bit 5); also gates the presort
    bool fused_update;                  // the fused update is allowed: no clustering, no boost, not bit 3 (then: rows to clean, and the kernel takes the shape)
    // "The host must see an update when it happens": files, the dumper and the update hook (host_tied); clustering and boost_posterior read the
    // device's counts.  The sequential-stream test mode joins in two spellings, and the fused branch asks a subset:
    bool host_tied;                     // dumper || on_update || resume_write
    bool sees_update;                   // ... || clustering || boost || seq_post: the count after the clean is fetched (seq_post = seq_mode with posteriors or
                                        //   equals: only then does a clean consume uniforms of the one stream, seq_consume)
    bool sees_update_seq;               // the same with seq_mode for seq_post: what forbids the deferred update (a sequential run's kernels follow the reference's order
                                        //   whatever it writes) and what finish_may_wait asks.  For finish_may_wait the wider spelling is an accident, kept: a sequential
                                        //   run without posteriors is told "may wait" for an update that does not
    bool sees_update_fused;             // host_tied || seq_post: the fused branch's own question -- clustering and boost never reach it (fused_update)
    PcCtlRead ctl;                      // when the whole control block is read at an update
    bool hook_late;                     // boost with posteriors: the dumper waits for this update's phantoms (nested_sampling.F90:325-336); the same rows are collected
    // The parallel contraction may run past an update trigger and have the update made afterwards, for the state at the trigger (pc_update.hip): a
    // nursery is then consumed in ONE launch instead of being cut where the reference updates.  Only when nothing on the host is tied to the moment
    // of an update and the fused update applies (bit 2: never).
    bool defer;
    // Pool mode (same conditions, likelihood on the device; bit 1: never): k_slice writes a nursery's babies into the phantom array itself, updates
    // invalidate phantoms where they lie, and the array is compacted only when it is full (pc_state.h).
    bool pool;
};
inline PcRunPlan pc_plan_run(const PcRunFacts &f)
{
    PcRunPlan p{};
    p.ablate = f.ablate; p.seq_mode = f.seq_mode;
    p.static_ok = f.fixed_nlive && f.force_general != 1;
    p.fast_ok = p.static_ok && f.fast_fits;
    p.par_ok = p.static_ok && f.force_general == 0 && f.par_fits;
    p.cl_ok = p.static_ok && f.force_general == 0 && !(f.ablate & PC_ABL_CONSUME_GENERAL);
    p.fused_update = !f.clustering && !f.boost && !(f.ablate & PC_ABL_NO_FUSED_UPDATE);
    const bool seq_post = f.seq_mode && f.posteriors;
    p.host_tied = f.dumper || f.on_update || f.resume_write;
    p.sees_update = p.host_tied || f.clustering || f.boost || seq_post;
    p.sees_update_seq = p.host_tied || f.clustering || f.boost || f.seq_mode;
    p.sees_update_fused = p.host_tied || seq_post;
    p.ctl = !p.sees_update ? PC_CTL_NONE : (f.clustering && !(p.host_tied || f.boost || seq_post)) ? PC_CTL_LATE : PC_CTL_EARLY;
    p.hook_late = f.boost && f.posteriors;
    p.defer = !(f.ablate & PC_ABL_NO_DEFER) && p.par_ok && !p.sees_update_seq && p.fused_update && f.fused_fits_one;
    p.pool = p.defer && !f.callback && !(f.ablate & PC_ABL_NO_POOL);
    return p;
}

// what a sampling launch of the run alone is counted under besides its kernel (live points, nurseries): run-time compiled kernels, of those the terms
// form of a source, a prior table evaluated on the device
struct PcLaunchTraits { bool rtc, src_terms, device_prior; };

// ---- a nursery ------------------------------------------------------------------------------------------------------------------------
struct PcNurseryFacts {
    bool in_step;                       // this run goes round by round with others of its device (Engine::co)
    bool other_active;                  // another run is in flight on the device
    bool callback;
    int D;
    bool ring;                          // a second buffer for bases drawn ahead exists
    bool slot_ready;                    // this nursery's bases were drawn ahead into its ring slot
    bool second_stream;                 // in step: the cohort has its second stream and the ring is two deep
    bool splittable, fusable, bases_t, slice_t;      // pc_nhats_splittable, pc_slice_fusable, pc_bases_t_ok, pc_slice_t_ok (the clusters there are now)
    bool cohort_general;                // what the cohort's launches for any device likelihood take (Engine::cohort_general_ok)
    PcLaunchTraits traits;
};
enum PcBases { PC_BASES_READY = 0,      // drawn on the side stream (or the cohort's second) while earlier nurseries were sampled and consumed: wait for them
               PC_BASES_PART1,          // part 1 of the split launch now, in front of the sampling kernel
               PC_BASES_PART1_STEP,     // ... written down for the cohort: one launch for all runs (CK_BASES; nDims <= 24)
               PC_BASES_NHATS_G,        // nDims 25 ... 64 in step: the whole kernel with the run in the grid (CK_NHATS_G; the halves are for a run on its own)
               PC_BASES_WHOLE };        // bases, seeds and whitening in one kernel of this run alone (no buffers, grades, the sequential mode, callbacks in step)
enum PcSampler { PC_SAMPLER_CALLBACK = 0,     // the device proposes, the host evaluates (pc_callback.hip)
                 PC_SAMPLER_LANE,       // next to other runs of the device (or bit 6): lane = chain (pc_slice_t.hip), the same numbers from 1/60 of the wavefronts
                 PC_SAMPLER_WAVE_STEP,  // in step, any device likelihood / several clusters: the one-run kernel with the run in the grid (CK_SLICE_G)
                 PC_SAMPLER_WAVE };     // a launch of this run alone: lane = coordinate
enum PcAhead { PC_AHEAD_NONE = 0,
               PC_AHEAD_STEP,           // in step: the next nursery's bases on the runs' second stream, next to this round's kernels (bases_ahead)
               PC_AHEAD_SIDE };         // a run that has the chip to itself: the nurseries to come on its side stream (side_prefetch); next to other runs the
                                        //   side streams would take from each other what they give
struct PcNurseryChoice {
    PcBases bases;
    bool packed;                        // PC_BASES_PART1: the lane-per-vector kernel (next to other runs, or bit 7)
    bool part2;                         // seeds + whitening as a launch of their own (else inside k_slice: fused)
    PcSampler sampler;
    bool fused;
    PcAhead ahead;
    PcLaunchTraits traits;
};
inline PcNurseryChoice pc_choose_nursery(const PcRunPlan &p, const PcNurseryFacts &f)
{
    PcNurseryChoice c{};
    c.traits = f.traits;
    const bool multi = f.in_step || f.other_active;
    const bool mid = f.D > 24 && f.D <= 64;
    const bool split = f.splittable && f.ring && !(mid && multi);      // the split launch and its ring of buffers are in use
    const bool general_step = f.in_step && !f.callback && f.cohort_general;
    if (split) {
        c.bases = f.slot_ready ? PC_BASES_READY : (f.in_step && f.bases_t) ? PC_BASES_PART1_STEP : PC_BASES_PART1;
        c.packed = c.bases == PC_BASES_PART1 && (multi || (p.ablate & PC_ABL_BASES_PACKED));
        c.fused = !f.callback && f.fusable;
        c.part2 = !c.fused;
    }
    else c.bases = (general_step && mid) ? PC_BASES_NHATS_G : PC_BASES_WHOLE;
    if (f.callback) c.sampler = PC_SAMPLER_CALLBACK;
    else if (c.fused && (multi || (p.ablate & PC_ABL_SLICE_LANE)) && f.slice_t) c.sampler = PC_SAMPLER_LANE;
    else if (general_step && (c.fused || !split)) c.sampler = PC_SAMPLER_WAVE_STEP;
    else c.sampler = PC_SAMPLER_WAVE;
    const bool step_kernel = c.sampler == PC_SAMPLER_LANE || c.sampler == PC_SAMPLER_WAVE_STEP;
    if (split && !multi) c.ahead = PC_AHEAD_SIDE;
    else if (f.in_step && step_kernel && c.fused && f.second_stream && f.bases_t) c.ahead = PC_AHEAD_STEP;
    return c;
}

// ---- a contraction --------------------------------------------------------------------------------------------------------------------
struct PcContractFacts {
    int ncluster, nursery_left;
    bool in_step, cohort_general;
    bool nn_lists;                      // the run has candidate lists (clustering) and PC_NN_LISTS_OFF is not set
    bool nn_valid;                      // ... made for this nursery already
    bool cl_fits, clp_fits;             // pc_consume_cl_fits, pc_consume_clp_fits for the clusters there are now
};
enum PcContract { PC_CONTRACT_PAR = 0,  // one cluster: the parallel contraction, which keeps the sorted order of the live set up to date itself
                  PC_CONTRACT_FAST,     // one cluster, a nursery beyond the parallel kernel: one wavefront (k_consume_fast)
                  PC_CONTRACT_CL_STEP,  // several clusters in step: lists, sort and the one-wave contraction once for all such runs (CK_NN, CK_SORT, CK_CONSUME_CL)
                  PC_CONTRACT_CL,       // several clusters, static number of live points, lists in place: the one-wave contraction (pc_clus.hip)
                  PC_CONTRACT_GENERAL };      // everything else -- and every launch under bit 5 -- : the general kernel, which is the arbiter
struct PcContractChoice {
    PcContract kind;
    // several clusters: rank the possible nearest neighbours of every baby still in the nursery once, on the whole chip; the serial contraction then
    // walks short lists instead of searching the live set
    bool want_nn;
    bool clp;                           // PC_CONTRACT_CL*: k_consume_clp (decisions in parallel), else the serial k_consume_cl (bit 10, or its LDS block does not fit)
};
inline PcContractChoice pc_choose_contract(const PcRunPlan &p, const PcContractFacts &f)
{
    PcContractChoice c{};
    if (p.par_ok && f.ncluster == 1) { c.kind = PC_CONTRACT_PAR; return c; }
    if (p.fast_ok && f.ncluster == 1) { c.kind = PC_CONTRACT_FAST; return c; }
    c.want_nn = f.ncluster > 1 && f.nn_lists && !f.nn_valid && !p.seq_mode && f.nursery_left > 1;
    const bool use_cl = p.cl_ok && (f.nn_valid || c.want_nn) && !p.seq_mode && f.ncluster > 1 && f.cl_fits;
    c.kind = !use_cl ? PC_CONTRACT_GENERAL : (f.in_step && f.cohort_general) ? PC_CONTRACT_CL_STEP : PC_CONTRACT_CL;
    c.clp = use_cl && f.clp_fits;
    return c;
}

// ---- an update ------------------------------------------------------------------------------------------------------------------------
struct PcUpdateFacts {
    bool rows;                          // there are phantoms to clean
    bool fused_fits;                    // pc_update_fused_ok for the clusters there are now
    int ncluster;
};
enum PcUpdate { PC_UPDATE_FUSED = 0,    // one cluster: clean + covariance + Cholesky by pc_update.hip (bit 16: as a chain of two launches)
                PC_UPDATE_STEPS };      // clean, covariances and Cholesky factors launch by launch (clustered runs, boost, nDims beyond the fused kernel)
struct PcUpdateChoice {
    PcUpdate kind;
    bool need_count;                    // the host waits for the count of surviving phantoms (else it is stale until the next read-back: no extra sync)
    PcCtlRead ctl; bool hook_late;      // (the plan's)
    bool may_wait;                      // round_finish may wait for the device in this update (Engine::finish_may_wait; `rows` is not asked)
};
inline PcUpdateChoice pc_choose_update(const PcRunPlan &p, const PcUpdateFacts &f)
{
    PcUpdateChoice c{};
    c.kind = (p.fused_update && f.rows && f.fused_fits) ? PC_UPDATE_FUSED : PC_UPDATE_STEPS;
    c.need_count = c.kind == PC_UPDATE_FUSED ? p.sees_update_fused : p.sees_update;
    c.ctl = p.ctl; c.hook_late = p.hook_late;
    c.may_wait = p.sees_update_seq || f.ncluster > 1 || !f.fused_fits;
    return c;
}

// ---- pchip_result.path[]: what each choice adds -----------------------------------------------------------------------------------------
inline void pc_count(long *path, const PcLaunchTraits &t)
{
    if (t.rtc) path[PCHIP_PATH_SOURCE_KERNELS]++;
    if (t.src_terms) path[PCHIP_PATH_SOURCE_TERMS]++;
    if (t.device_prior) path[PCHIP_PATH_DEVICE_PRIOR]++;
}
inline void pc_count(long *path, const PcNurseryChoice &c)
{
    switch (c.sampler) {
    case PC_SAMPLER_CALLBACK: break;
    case PC_SAMPLER_LANE: path[PCHIP_PATH_SLICE_LANE]++; break;
    // (a launch for the runs in step takes no prior table and, through pchip_run_repeats, no source: of the three traits only the first is asked)
    case PC_SAMPLER_WAVE_STEP: path[PCHIP_PATH_SLICE_WAVE]++; pc_count(path, PcLaunchTraits{c.traits.rtc, false, false}); break;
    case PC_SAMPLER_WAVE: path[PCHIP_PATH_SLICE_WAVE]++; pc_count(path, c.traits); break;
    }
}
// ... and what a launch for the runs in step adds now that it takes a source and a device prior (pchip_run_in_step): the other two traits.  (A function
// of its own: pc_count above is what it was, tests/test_run_plan.py.)  Whether the launch was shared is known where it is made: Cohort::flush
// counts PCHIP_PATH_SLICE_STEP.
inline void pc_count_step(long *path, const PcNurseryChoice &c)
{
    if (c.sampler == PC_SAMPLER_WAVE_STEP) pc_count(path, PcLaunchTraits{false, c.traits.src_terms, c.traits.device_prior});
}
inline void pc_count(long *path, const PcContractChoice &c)
{
    if (c.want_nn) path[PCHIP_PATH_NN_LISTS]++;
    switch (c.kind) {
    case PC_CONTRACT_PAR: path[PCHIP_PATH_CONSUME_PAR]++; break;
    case PC_CONTRACT_FAST: path[PCHIP_PATH_CONSUME_FAST]++; break;
    case PC_CONTRACT_CL_STEP: case PC_CONTRACT_CL: path[c.clp ? PCHIP_PATH_CONSUME_CL : PCHIP_PATH_CONSUME_CL_SERIAL]++; break;
    case PC_CONTRACT_GENERAL: path[PCHIP_PATH_CONSUME_GENERAL]++; break;
    }
}
inline void pc_count(long *path, const PcUpdateChoice &c) { path[c.kind == PC_UPDATE_FUSED ? PCHIP_PATH_UPDATE_FUSED : PCHIP_PATH_UPDATE_STEPS]++; }
// live points beyond nlive (nprior > nlive, a resume file written with more): killed by the general kernel before the first round, nested_sampling.F90:201-205
struct PcTrimLive {};
inline void pc_count(long *path, const PcTrimLive &) { path[PCHIP_PATH_CONSUME_GENERAL]++; }
