// pc_tick.h -- the runs of a group in step whose likelihood is the caller's DEVICE batch callback: what they share while a nursery is sampled.
//
// Host only.  Included by pc_engine.hip alone, behind Engine and ahead of pc_step.h, whose tick phase (StepGroup::enqueue_as_fibers) drives it.
// (tools/dev/step_record.hip stands an empty TickGroup in: its scripted runs have no callback.)  It needs of the including file: Engine --
// its members B, S, st, stop, dev_batch, tick_asked, tick_want, tick_count, tick_bind, device_call, tick_answered --, RunBlocks (pc_blocks.h),
// pc_launch.h and HIPCHK.
//
// The library's own evaluator of a batched quadratic form (pchip_source_create_quad_batch, Engine::quad_batch_call) takes the caller's place
// unchanged: the group's first run that ticked evaluates the rows of all of them, from its own copy of the handle's block.
//
// One block of answers for all runs, sized for the sum of their chains a nursery; every run's db_cube / db_theta / db_phi / db_logL point at
// it, so a run's tick finds its answers at the GLOBAL ranks the pack leaves in the run's rank array, with no change to the tick's indexing.
// A tick of the group is: the ticks of the runs that wait (Cohort::flush, CK_TICK: one launch), pack(), ONE stream wait, answer().
// The rows are ordered by run -- the order of `seeds` within the group -- and inside a run by ascending chain: the solo order, concatenated.
#pragma once
#include <vector>

namespace {

struct TickGroup {
    RunBlocks blocks;                              // the group's ledger: the one block and the words of the pack
    std::vector<Engine *> runs;                    // by their place in the group (null: not one of the rounds)
    double *cube = nullptr, *theta = nullptr, *phi = nullptr, *logL = nullptr;
    PcParkRun *asks = nullptr, *asks_dev = nullptr;      // pinned, read by the pack's kernels: the runs that ticked, in group order
    int *d_count = nullptr, *hp_count = nullptr, *hp_count_dev = nullptr;      // counts [64] on the device; pinned: each run's count, then the total
    int who[PC_PARK_MAX_RUNS]; int nask = 0;
    bool on = false;

    // the likelihoods whose runs tick: a callback (behind the caller's device batch callback: pc_run_many's caller has checked that one is
    // registered) and a batched quadratic form (pchip_source_create_quad_batch), whose evaluator is the library's own
    static int quad_batch_nres(const pchip_like *like) { int nres = 0; (void)pc_quad_batch_refusal("pchip_run_in_step", like, nullptr, &nres); return nres; }
    static bool ticks(const pchip_like *like) { return like && (like->kind == PCHIP_LIKE_CALLBACK || quad_batch_nres(like) > 0); }

    // Assumes the runs set up and begun (their live points made, each by calls of its own: nprior rows a run), the stream idle.  Leaves the
    // one block allocated and every run bound to it.
    void set_up(const std::vector<Engine *> &E, const std::vector<char> &live, int n)
    {
        size_t rows = 0; int D = 1, pd = 1;
        runs.assign((size_t)n, nullptr);
        for (int k = 0; k < n; ++k) if (live[k] && E[k] && E[k]->dev_batch) { runs[(size_t)k] = E[k]; rows += (size_t)E[k]->B; D = E[k]->S.D; pd = std::max(1, E[k]->S.nDer); }
        if (!rows) return;
        if (n > PC_PARK_MAX_RUNS) throw EngineError{PC_RC_LIMIT, "device batch callbacks in step: at most 64 runs a group"};
        cube = blocks.dev<double>(rows * D); theta = blocks.dev<double>(rows * D); phi = blocks.dev<double>(rows * pd); logL = blocks.dev<double>(rows);
        d_count = blocks.dev<int>(PC_PARK_MAX_RUNS);
        asks = blocks.pin<PcParkRun>(PC_PARK_MAX_RUNS); hp_count = blocks.pin<int>(PC_PARK_MAX_RUNS + 1);
        { void *dp = nullptr; HIPCHK(hipHostGetDevicePointer(&dp, asks, 0)); asks_dev = (PcParkRun *)dp; }
        { void *dp = nullptr; HIPCHK(hipHostGetDevicePointer(&dp, hp_count, 0)); hp_count_dev = (int *)dp; }
        HIPCHK(hipMemset(phi, 0, sizeof(double) * rows * pd));      // (no derived parameters: a column nobody writes)
        for (Engine *e : runs) if (e) e->tick_bind(cube, theta, phi, logL);
        on = true;
    }

    // Assumes the ticks of the runs that asked launched on `st`.  Leaves the pack enqueued behind them: their parked proposals in the one block,
    // global ranks in their rank arrays, their counts and the total on the way to the pinned words.  Nothing where nobody asked.
    void pack(hipStream_t st)
    {
        nask = 0;
        int max_chains = 0, D = 1;
        for (size_t k = 0; k < runs.size(); ++k) {
            Engine *e = runs[k];
            if (!e || !e->tick_asked) continue;
            asks[nask] = e->tick_want; who[nask++] = (int)k;
            max_chains = std::max(max_chains, e->tick_want.nchains); D = e->S.D;
        }
        if (!nask) return;
        if (pc_launch_park_pack_many(nask, asks_dev, max_chains, D, d_count, hp_count_dev, cube, st)) throw EngineError{PC_RC_DEVICE, "the pack of a group's parked proposals could not be launched"};
    }

    // Assumes the stream waited for.  Leaves every run that asked told its count; if there are rows at all, the engine's prior on the whole
    // block and ONE call of the caller's function enqueued for them, counted by every run with rows in it.  A non-zero return stops every run.
    void answer()
    {
        if (!nask) return;
        const int total = ((volatile int *)hp_count)[nask];
        for (int a = 0; a < nask; ++a) { Engine *e = runs[(size_t)who[a]]; e->tick_count = ((volatile int *)hp_count)[a]; e->tick_asked = false; }
        const int na = nask; nask = 0;
        if (total <= 0) return;
        Engine *first = runs[(size_t)who[0]];
        for (int a = 0; a < na; ++a) { Engine *e = runs[(size_t)who[a]]; if (e->tick_count > 0) e->tick_answered(e->tick_count); }
        first->device_call(total);
        if (first->stop.load(std::memory_order_relaxed)) for (Engine *e : runs) if (e) e->stop.store(1);
    }

    // a run that is over leaves the group (its engine is deleted by its ending's thread)
    void leave(int k) { if ((size_t)k < runs.size()) runs[(size_t)k] = nullptr; }
    // what a failed phase left half done is forgotten
    void drop() { nask = 0; for (Engine *e : runs) if (e) e->tick_asked = false; }
    // Assumes the group's stream idle and its runs destroyed.  Leaves nothing held.
    void release() { blocks.release_all(); runs.clear(); on = false; }
};

}  // namespace
