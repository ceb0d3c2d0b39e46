// pc_step.h -- the driver of one group of runs in step: pc_run_many, and the phases it goes through for a group (StepGroup).
//
// Host only.  Included by pc_engine.hip alone, behind Engine (and by tools/dev/step_record.hip, which stands a scripted Engine and recorders in
// for everything below and compares what the driver does with the pc_run_many of the commit before this header existed, b330d9b:
// tests/test_step_record.py).  The including file provides, before the include: polychord_hip.h, pc_plan.h (pc_env), pc_fiber.h, pc_cohort.h;
// the HIP device, stream, event and copy calls, HIPCHK around them, EngineError and the PC_RC_* codes; and
//   of Engine, these members and no others:
//     co, fib, dev, st_side, r_rc, d_total
//     setup, begin, compact_wanted, compact_record, compact_finish
//     round_enqueue, round_ready, finish_may_wait, round_finish
//     end_a, end_a2, end_wait_aside, end_b, destroy
//   TickGroup (pc_tick.h: what runs through the caller's device batch callback share): ticks, on, set_up, pack, answer, leave, drop, release
//   these services:
//     hpool()                      get_stream, put_stream, take_stream_if, get_sync_event, put_sync_event
//     sclasses()                   known, classify: a stream's hardware-queue class
//     cstreams(), CohortLease      the classes the groups at work on a device hold, and this group's share of them
//     stream_avoiding, stream_beside
//     halloc / hfree, pchip_result_free
//     for the PC_DEBUG=5 report alone: the g_dbg_* counters, dcache().cached, hcache().cached
//
// The calling thread drives the group: every phase of the round is gone through for all runs before anything is launched, then each kernel of
// the phase once for all (Cohort).  A phase reads and writes the members of StepGroup and nothing else; its comment says what it assumes and
// what it leaves.
#pragma once
#include <vector>
#include <string>
#include <memory>
#include <atomic>
#include <mutex>
#include <thread>
#include <chrono>
#include <algorithm>
#include <exception>
#include <cstdio>
#include <cstring>

namespace {

// where a group's wall time went (PC_DEBUG=5): each phase adds to its own figures, report() prints them all
struct StepTimes {
    using clk = std::chrono::steady_clock;
    static clk::time_point now() { return clk::now(); }
    static double sec(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }
    clk::time_point t_pre = now(), t0 = t_pre;      // the group's start, and its start once it has its streams
    double setup_first = 0, begin = 0, comp = 0, enq = 0, fl = 0, wait = 0, fin = 0, fwait = 0, end_dev = 0, end = 0;
    long rounds = 0, n_fwait = 0; int n_comp_pass = 0;
    void report(int n, size_t n_endings, const Cohort &co) const
    {
        std::fprintf(stderr, "polychord_hip dbg cohort: of enqueue: nursery %.2f ms (compaction %.2f), capacity %.2f\n", g_dbg_nursery_ns.exchange(0) * 1e-6, g_dbg_compact_ns.exchange(0) * 1e-6, g_dbg_capacity_ns.exchange(0) * 1e-6);
        std::fprintf(stderr, "polychord_hip dbg cohort: %zu ending batches: events %.2f ms, results %.2f ms, teardown %.2f ms (summed over threads); the block caches hold %.2f GB of device and %.2f GB of pinned memory; teardown: device blocks %.2f, the rest %.2f ms\n", n_endings, g_dbg_evwait_ns.exchange(0) * 1e-6, g_dbg_endb_ns.exchange(0) * 1e-6, g_dbg_destroy_ns.exchange(0) * 1e-6, dcache().cached / 1073741824.0, hcache().cached / 1073741824.0, g_dbg_d1.exchange(0) * 1e-6, g_dbg_d2.exchange(0) * 1e-6);
        std::fprintf(stderr, "polychord_hip dbg cohort: the first run's set-up and live points %.2f ms\n", setup_first * 1e3);
        std::fprintf(stderr, "polychord_hip dbg cohort: trips to the driver: %lld device blocks (%.2f ms), %lld pinned blocks (%.2f ms), %lld streams (%.2f ms)\n", g_dbg_miss_n[0].exchange(0), g_dbg_miss_ns[0].exchange(0) * 1e-6, g_dbg_miss_n[1].exchange(0), g_dbg_miss_ns[1].exchange(0) * 1e-6, g_dbg_mk_stream_n.exchange(0), g_dbg_mk_stream_ns.exchange(0) * 1e-6);
        std::fprintf(stderr, "polychord_hip dbg cohort: %d runs, %ld rounds, streams %.2f ms, wall %.2f ms (setup + begin %.2f, compactions %.2f in %d passes, enqueue %.2f, finish %.2f, launches %.2f, waiting for the device %.2f, the endings' requests %.2f, waiting for the endings %.2f); %ld records launched together, %ld one by one\n", n, rounds, sec(t_pre, t0) * 1e3,
                     sec(t0, now()) * 1e3, begin * 1e3, comp * 1e3, n_comp_pass, enq * 1e3, fin * 1e3, fl * 1e3, wait * 1e3, end_dev * 1e3, end * 1e3, co.n_fused, co.n_single);
        std::fprintf(stderr, "polychord_hip dbg cohort: of finish: %ld shared waits, %.2f ms\n", n_fwait, fwait * 1e3);
    }
};

struct StepGroup {
    // the runs of seeds[0 .. n) on `device`, their results into results[0 .. n)
    const pchip_settings *s; const pchip_like *like; const pchip_prior *prior; const int *seeds; int device; pchip_result *results;
    int n;                                        // runs of the group (set_up_runs makes it smaller when only some fit)
    int worst = 0;                                // the first failing run's code: the rounds stop at once
    int nlive = 0;                                // runs whose rounds go on
    int devq;                                     // the HIP device of the calling thread, as an index of the tables by device
    Cohort co;
    CohortLease lease;
    std::vector<Engine *> E;                      // (sized by set_up_runs) null: not set up, or ended and deleted
    std::vector<char> live, enq;                  // live: its rounds go on; enq: it has a round under way
    std::vector<Fiber> fibs;
    // runs that are over, handed to a thread of their own: it waits for the two events, then makes the host's half of their endings
    struct EndBatch { std::vector<int> fin, rcs; hipEvent_t ev = nullptr, ev2 = nullptr; int dev = 0; std::thread th; };
    std::vector<std::unique_ptr<EndBatch>> endings;
    int *h_totals = nullptr; size_t totals_cap = 0;      // compact_full's rows in use, one pinned word per run
    // the likelihood is the caller's device batch callback: the runs' ticks go together (enqueue_as_fibers), their answers share one block (tg),
    // and the caller's function is called on this thread alone
    // (or the library's own evaluator of a batched quadratic form, which goes the same way: TickGroup::ticks says which likelihoods do)
    const bool ticking = TickGroup::ticks(like);
    TickGroup tg;
    const bool fibers_on = !pc_env().cohort_fibers_off, prof = pc_env().debug == 5;
    StepTimes t;

    static int current_device() { int d = 0; (void)hipGetDevice(&d); return d; }
    StepGroup(const pchip_settings *s_, const pchip_like *like_, const pchip_prior *prior_, const int *seeds_, int device_, pchip_result *results_, int n_)
        : s(s_), like(like_), prior(prior_), seeds(seeds_), device(device_), results(results_), n(n_), devq(current_device() & 63), lease(devq) {}      // (nothing here throws: the phases do, inside the caller's handlers)
    ~StepGroup() { join_endings(); release(); }

    // Assumes nothing.  Leaves the cohort's four streams by hardware-queue class -- co.st, and co.st2 / co.stc[] unless switched off --, the
    // two events of the second stream, and the classes of the first two entered in cstreams() under the lease.
    void pick_streams()
    {
        const bool side_off = pc_env().cohort_side_off;
        // (a main stream whose hardware queue is known already, if the pool has one: the side stream is then picked without a test --
        //  a test is a millisecond, several once PyTorch lives in the process, and the pool's first stream was a different one of
        //  the engines' copy streams at every call)
        // (and the pair of the call before, if the pool still has it: whatever the runtime sets up for a stream at its first copy or
        //  launch is then there -- a call's first wait was 10 ... 24 ms now and then while the pair changed from call to call)
        static std::mutex last_m; static hipStream_t last_st[64] = {nullptr}, last_st2[64] = {nullptr};
        int cls_main = -1, cls_side = -1;
        bool loaded;                                              // another group is at work on this device: no class tests now
        {
            hipStream_t want, want2;
            { std::lock_guard<std::mutex> g(last_m); want = last_st[devq]; want2 = last_st2[devq]; }
            std::lock_guard<std::mutex> gq(cstreams().m);             // (one group at a time picks: what it takes the next one avoids)
            std::vector<int> busy = cstreams().busy(devq);
            loaded = !busy.empty();
            // (more groups than hardware queues can keep apart: at least not on another group's MAIN stream's queue)
            if (busy.size() >= 4) busy = cstreams().busy(devq, true);
            auto free_cls = [&](hipStream_t x) { const int c = sclasses().known(x); return c >= 0 && std::find(busy.begin(), busy.end(), c) == busy.end(); };
            if (want) co.st = hpool().take_stream_if([&](hipStream_t x) { return x == want && (busy.empty() || free_cls(x)); });
            if (!co.st) co.st = hpool().take_stream_if([&](hipStream_t x) { return busy.empty() ? sclasses().known(x) >= 0 : free_cls(x); });
            if (!co.st) co.st = busy.empty() ? hpool().get_stream() : stream_avoiding(busy, loaded);
            const auto tp1 = t.now();
            if (!busy.empty() || !side_off) cls_main = loaded ? sclasses().known(co.st) : sclasses().classify(co.st);
            if (!side_off) {
                if (cls_main >= 0) busy.push_back(cls_main);
                if (co.st == want && want2) co.st2 = hpool().take_stream_if([&](hipStream_t x) { return x == want2 && free_cls(x); });
                if (!co.st2) co.st2 = stream_avoiding(busy, loaded);
                cls_side = loaded ? sclasses().known(co.st2) : sclasses().classify(co.st2);
            }
            cstreams().take(devq, cls_main, true); cstreams().take(devq, cls_side); lease.hold(cls_main, cls_side);
            { std::lock_guard<std::mutex> g(last_m); last_st[devq] = co.st; last_st2[devq] = co.st2; }
            if (prof) std::fprintf(stderr, "polychord_hip dbg cohort: main stream %.2f ms, side stream %.2f ms\n", t.sec(t.t_pre, tp1) * 1e3, t.sec(tp1, t.now()) * 1e3);
        }
        if (co.st2) { co.ev_up = hpool().get_sync_event(); co.ev_next = hpool().get_sync_event(); }
        if (!pc_env().cohort_copy_streams_off) { co.stc[0] = stream_beside({co.st, co.st2}, loaded); co.stc[1] = stream_beside({co.st, co.st2, co.stc[0]}, loaded); }
        t.t0 = t.now();
    }

    // Assumes the streams.  Leaves E[k] set up and begun and live[k] = 1 for the runs that go into the rounds, nlive their number; n smaller
    // when the device's memory holds only the first few of the runs (the caller starts the next group at the first that did not fit).
    // Throws what the first run's set-up throws, and whatever a later one's throws other than for want of memory.
    void set_up_runs()
    {
        // set-up and live points of the runs: the first one by itself (a run that does not fit, or fails, alone is the
        // call's failure), then the others -- a tenth of a millisecond of host work each, 7 ms of sixty-four runs' 175.
        // (Shared out among four threads it was TWICE as long -- 13 ms -- the runtime's calls queue for one another:
        //  PC_COHORT_SETUP_THREADS, one by default)
        E = std::vector<Engine *>((size_t)n, nullptr); live = std::vector<char>((size_t)n, 0); enq = std::vector<char>((size_t)n, 0);
        std::vector<int> rc_begin((size_t)n, -1), err((size_t)n, 0);
        std::vector<std::string> errmsg((size_t)n);
        std::atomic<bool> failed{false};
        const int devnow = current_device();
        auto setup_one = [&](int k) {
            E[k] = new Engine; E[k]->co = &co;
            pchip_settings c = *s; c.seed = seeds[k]; c.device = device;
            const auto q0 = t.now();
            try { E[k]->setup(c, *like, *prior); rc_begin[k] = E[k]->begin(); }
            catch (const EngineError &e) { err[k] = e.code ? e.code : PC_RC_DEVICE; errmsg[k] = e.msg; failed = true; }
            catch (const std::bad_alloc &) { err[k] = PC_RC_MEMORY; errmsg[k] = "out of host memory"; failed = true; }
            if (k == 0) t.setup_first = t.sec(q0, t.now());
        };
        const auto b0 = t.now();
        setup_one(0);
        const int setup_threads = pc_env().cohort_setup_threads;
        if (n > 1 && !failed) {
            std::atomic<int> nextk{1};
            auto worker = [&] { (void)hipSetDevice(devnow); for (int k; !failed && (k = nextk.fetch_add(1)) < n;) setup_one(k); };
            std::vector<std::thread> th;
            for (int w = 1; w < std::min(setup_threads, n - 1) && n >= 8 && !ticking; ++w) th.emplace_back(worker);      // (ticking: the live points are the caller's function at work, on this thread)
            worker();
            for (auto &w : th) w.join();
        }
        t.begin += t.sec(b0, t.now());
        for (int k = 0; k < n; ++k) {
            if (!err[k] && E[k]) continue;
            if (err[k] && (err[k] != PC_RC_MEMORY || k == 0)) throw EngineError{err[k], errmsg[k]};
            // no memory for one more run of this size next to the k that are set up: those go in step, the others after them
            (void)hipGetLastError();
            for (int j = k; j < n; ++j) if (E[j]) { try { E[j]->destroy(); } catch (...) {} delete E[j]; E[j] = nullptr; }
            n = k;
            break;
        }
        for (int k = 0; k < n; ++k) {
            const int rc = rc_begin[k];
            if (rc >= 0) {      // over before its first round
                pchip_result_free(&results[k]);
                if (!worst) worst = rc ? rc : PC_RC_DEVICE;
                E[k]->destroy(); delete E[k]; E[k] = nullptr;
                continue;
            }
            live[k] = 1; nlive++;
        }
        if (ticking && nlive > 0) tg.set_up(E, live, n);
    }

    // Assumes the live runs between two rounds.  Leaves the phantom arrays that were full compacted, together, with one wait for all.
    // (Only the full ones: taking the arrays that are more than half full along -- the runs fill theirs at slightly different rates, and a
    // pass a round later is another wait of the whole cohort -- kept the passes at three a call, and changed the last bits of some runs:
    // the update's partial sums are grouped by the array's extent, so a run must compact exactly when it would alone.
    // tools/dev/fuzz_in_step.py found it)
    void compact_full()
    {
        int nc = 0;
        for (int k = 0; k < n; ++k) if (live[k] && E[k]->compact_wanted()) nc++;
        if (!nc) return;
        const auto c0 = t.now();
        std::vector<char> cmp((size_t)n, 0);
        for (int k = 0; k < n; ++k) if (live[k] && E[k]->compact_wanted()) { cmp[k] = 1; E[k]->compact_record(); }
        co.flush();
        if ((size_t)n > totals_cap) { if (h_totals) hfree(h_totals); h_totals = halloc<int>((size_t)n); totals_cap = (size_t)n; }
        for (int k = 0; k < n; ++k) if (cmp[k]) HIPCHK(hipMemcpyAsync(&h_totals[k], E[k]->d_total, sizeof(int), hipMemcpyDeviceToHost, co.st));
        HIPCHK(hipStreamSynchronize(co.st));
        for (int k = 0; k < n; ++k) if (cmp[k]) E[k]->compact_finish(h_totals[k]);
        t.comp += t.sec(c0, t.now()); t.n_comp_pass++;
    }

    // Assumes the live runs between two rounds.  Leaves enq[k] = 1 for the runs that wrote a round down, and the round launched.
    void enqueue_round()
    {
        const auto a0 = t.now();
        if (tg.on) enqueue_as_fibers();
        else for (int k = 0; k < n; ++k) enq[k] = (live[k] && E[k]->round_enqueue()) ? 1 : 0;
        const auto a1 = t.now(); t.enq += t.sec(a0, a1);
        co.flush(); t.fl += t.sec(a1, t.now());
    }
    // ... round_enqueue of the live runs, each as a fiber, where a fresh nursery is sampled through the caller's device batch callback.
    // Assumes tg set up (every run's answers in the group's one block).  A run at a fresh nursery writes a tick down, says where its flags,
    // proposals and ranks are, and yields; a run in the middle of a nursery writes its round down and is done at once.  Between two resumes,
    // for all runs that wait: one launch of their ticks (and of whatever else was written down), one pack of their parked proposals into the
    // one block, one wait, the prior and ONE call of the caller's function on this thread if the pack found rows at all.  A run whose count
    // comes back zero is through with its nursery: it leaves the ticks, writes the rest of its round down and waits for the phase's end.
    // Leaves enq[k] as enqueue_round says, the last records written down and not launched.  When a run throws, or the pack or the call
    // does, the others are unwound as in finish_as_fibers and it is rethrown.
    void enqueue_as_fibers()
    {
        std::vector<int> wk;
        for (int k = 0; k < n; ++k) { enq[k] = 0; if (live[k]) wk.push_back(k); }
        if (fibs.size() < wk.size()) fibs.resize(wk.size());
        std::vector<char> ok(wk.size(), 0);
        for (size_t a = 0; a < wk.size(); ++a) {
            Fiber &f = fibs[a];
            f.make_stack();
            f.started = false; f.done = false; f.cancel = false; f.err = nullptr;
            Engine *e = E[wk[a]]; char *okp = &ok[a];
            f.fn = [e, okp] { *okp = e->round_enqueue() ? 1 : 0; };
            e->fib = &f;
        }
        std::exception_ptr first_err;
        for (;;) {
            bool waiting = false;
            for (size_t a = 0; a < wk.size(); ++a) {
                Fiber &f = fibs[a];
                if (f.done) continue;
                f.resume();
                if (f.err && !first_err) first_err = f.err;
                if (!f.done) waiting = true;
            }
            if (first_err || !waiting) break;
            const auto w0 = t.now();
            try {
                co.flush();
                tg.pack(co.st);
                pc_wait_stream(co.st);
                tg.answer();
            } catch (...) { first_err = std::current_exception(); break; }
            t.fwait += t.sec(w0, t.now()); t.n_fwait++;
        }
        if (first_err) {
            co.drop_pending(); tg.drop();
            for (size_t a = 0; a < wk.size(); ++a) {
                Fiber &f = fibs[a];
                if (f.started && !f.done) { f.cancel = true; f.resume(); }
            }
            co.drop_pending(); tg.drop();
        }
        for (size_t a = 0; a < wk.size(); ++a) { E[wk[a]]->fib = nullptr; enq[wk[a]] = ok[a]; }
        if (first_err) std::rethrow_exception(first_err);
    }

    // Assumes the round launched.  Leaves every run with a round under way told by the device what the round did.
    void await_round()
    {
        const auto w0 = t.now();
        for (int k = 0; k < n; ++k) if (enq[k]) while (!E[k]->round_ready()) __builtin_ia32_pause();
        t.wait += t.sec(w0, t.now());
    }

    // Assumes every run with a round under way knows what the round did.  Leaves the round finished (updates made, what they launch launched)
    // and enq[k] = 0 for the runs that are over.  A run whose update has to wait for the device in the middle (clustering, files, hooks)
    // makes it as a fiber of this thread; the others at once.
    void finish_round()
    {
        const auto a0 = t.now();
        std::vector<int> wk;
        for (int k = 0; k < n; ++k) {
            if (!enq[k]) continue;
            if (fibers_on && E[k]->finish_may_wait()) wk.push_back(k);
            else if (!E[k]->round_finish()) enq[k] = 0;
        }
        if (!wk.empty()) finish_as_fibers(wk);
        const auto a1 = t.now(); t.fin += t.sec(a0, a1);
        co.flush(); t.fl += t.sec(a1, t.now());
        t.rounds++;
    }
    // ... round_finish of the runs wk, each as a fiber: they share flushes and waits.  When one throws, the others are unwound and it is rethrown.
    void finish_as_fibers(const std::vector<int> &wk)
    {
        if (fibs.size() < wk.size()) fibs.resize(wk.size());
        std::vector<char> ok(wk.size(), 1);
        for (size_t a = 0; a < wk.size(); ++a) {
            Fiber &f = fibs[a];
            f.make_stack();
            f.started = false; f.done = false; f.cancel = false; f.err = nullptr;
            Engine *e = E[wk[a]]; char *okp = &ok[a];
            f.fn = [e, okp] { *okp = e->round_finish() ? 1 : 0; };
            e->fib = &f;
        }
        std::exception_ptr first_err;
        for (;;) {
            bool waiting = false;
            for (size_t a = 0; a < wk.size(); ++a) {
                Fiber &f = fibs[a];
                if (f.done) continue;
                f.resume();
                if (f.err && !first_err) first_err = f.err;
                if (!f.done) waiting = true;
            }
            if (first_err || !waiting) break;
            // one launch of what they all wrote down, one wait for all of them
            const auto w0 = t.now();
            co.flush();
            pc_wait_stream(co.st);
            t.fwait += t.sec(w0, t.now()); t.n_fwait++;
        }
        if (first_err) {
            // the fibers still suspended hold locals, pinned blocks and copies written down for a flush that will not come: what
            // they wrote down is dropped, and each is resumed once more with the cancel flag -- its wait throws, its frames unwind
            co.drop_pending();
            for (size_t a = 0; a < wk.size(); ++a) {
                Fiber &f = fibs[a];
                if (f.started && !f.done) { f.cancel = true; f.resume(); }
            }
            co.drop_pending();
        }
        for (size_t a = 0; a < wk.size(); ++a) { E[wk[a]]->fib = nullptr; if (!ok[a]) enq[wk[a]] = 0; }
        if (first_err) std::rethrow_exception(first_err);
    }

    // Assumes the round finished.  Leaves the runs that are over (live, no round under way) out of the rounds: their kill-off in one launch,
    // what their results need asked of the device behind it, and the rest handed to a thread (EndBatch).  Nobody waits here: the thread
    // takes the batch from there while the runs that are left go on with their rounds.  A run that failed stops the others at once (worst).
    void end_finished()
    {
        bool any_done = false;
        for (int k = 0; k < n; ++k) any_done = any_done || (live[k] && !enq[k]);
        if (!any_done) return;
        const auto e0 = t.now();
        co.flush();
        for (int k = 0; k < n; ++k) if (live[k] && !enq[k] && !E[k]->r_rc) E[k]->end_a(true);
        co.flush();
        for (int k = 0; k < n; ++k) if (live[k] && !enq[k] && !E[k]->r_rc) E[k]->end_a2();
        endings.emplace_back(new EndBatch);
        EndBatch *eb = endings.back().get();
        for (int k = 0; k < n; ++k) if (live[k] && !enq[k]) eb->fin.push_back(k);
        eb->rcs.assign(eb->fin.size(), 0);
        eb->dev = E[eb->fin[0]]->dev;
        eb->ev = hpool().get_sync_event(); HIPCHK(hipEventRecord(eb->ev, co.st));
        if (co.st2) { eb->ev2 = hpool().get_sync_event(); HIPCHK(hipEventRecord(eb->ev2, co.st2)); }      // (bases drawn ahead for a run that is over: not into freed memory)
        for (int k : eb->fin) { live[k] = 0; nlive--; tg.leave(k); if (E[k]->r_rc && !worst) worst = E[k]->r_rc; }
        eb->th = std::thread([this, eb] { end_batch(*eb); });
        t.end_dev += t.sec(e0, t.now());
    }
    // ... the batch's thread: two events, then the host's half of the endings -- results, buffers given back, a third of a millisecond per
    // run, shared out among a few threads.  It touches E[k] and results[k] of the batch's runs and nothing else of the group.
    void end_batch(EndBatch &eb)
    {
        using clk = std::chrono::steady_clock;
        auto ns = [](clk::time_point a, clk::time_point b) { return std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count(); };
        (void)hipSetDevice(eb.dev);
        const auto w0 = clk::now();
        const hipError_t w1 = hipEventSynchronize(eb.ev), w2 = eb.ev2 ? hipEventSynchronize(eb.ev2) : hipSuccess;
        g_dbg_evwait_ns += ns(w0, clk::now());
        auto finish_one = [&](size_t a) {
            const int k = eb.fin[a];
            int r = E[k]->r_rc;
            if (!r && (w1 != hipSuccess || w2 != hipSuccess)) r = PC_RC_DEVICE;
            const auto q0 = clk::now();
            if (!r) {
                try { E[k]->end_wait_aside(); r = E[k]->end_b(&results[k]); }
                catch (const EngineError &e) { std::fprintf(stderr, "polychord_hip: %s\n", e.msg.c_str()); r = e.code; }
                catch (const std::bad_alloc &) { r = PC_RC_MEMORY; }
            }
            const auto q1 = clk::now();
            if (r != 0) pchip_result_free(&results[k]);
            try { E[k]->destroy(r == 0 && E[k]->st_side == nullptr); } catch (...) {}      // (end_b has waited for the copy stream, this thread for the cohort's two)
            delete E[k]; E[k] = nullptr; eb.rcs[a] = r;
            g_dbg_endb_ns += ns(q0, q1);
            g_dbg_destroy_ns += ns(q1, clk::now());
        };
        const size_t nth = std::min<size_t>(eb.fin.size(), 8);
        if (nth <= 1) { for (size_t a = 0; a < eb.fin.size(); ++a) finish_one(a); }
        else {
            std::atomic<size_t> nexta{0};
            auto worker = [&] { (void)hipSetDevice(eb.dev); for (size_t a; (a = nexta.fetch_add(1)) < eb.fin.size();) finish_one(a); };
            std::vector<std::thread> th;
            for (size_t w = 1; w < nth; ++w) th.emplace_back(worker);
            worker();
            for (auto &w : th) w.join();
        }
    }

    // Assumes nothing (called on every path, a second time by the destructor).  Leaves no ending under way, the batches' codes in worst and
    // their events given back.
    void join_endings()
    {
        const auto e0 = t.now();
        for (auto &eb : endings) {
            if (eb->th.joinable()) eb->th.join();
            for (int r : eb->rcs) if (r != 0 && !worst) worst = r;
            for (hipEvent_t *e : {&eb->ev, &eb->ev2}) if (*e) { hpool().put_sync_event(*e); *e = nullptr; }
        }
        t.end += t.sec(e0, t.now());
    }

    // Assumes no ending under way.  Leaves nothing held: the runs still there (a failed call's) destroyed and their results freed, the
    // fibers' stacks, the cohort's blocks and events, h_totals, the tick group's block, the lease and the streams given back, each stream idle when it goes.
    // The PC_DEBUG=5 report is made in between, once the side stream is idle and the last engine destroyed: its wall time and its teardown
    // figures take those in, and nothing of them is left for the next group's report.
    void release()
    {
        if (co.st2) (void)hipStreamSynchronize(co.st2);
        for (int k = 0; k < (int)E.size(); ++k) if (E[k]) { pchip_result_free(&results[k]); try { E[k]->destroy(); } catch (...) {} delete E[k]; E[k] = nullptr; }
        if (prof) t.report(n, endings.size(), co);
        for (Fiber &f : fibs) f.free_stack();
        co.destroy();
        if (h_totals) { hfree(h_totals); h_totals = nullptr; }
        if (co.st) (void)hipStreamSynchronize(co.st);
        tg.release();
        lease.release();
        if (co.st) { hpool().put_stream(co.st); co.st = nullptr; }
        if (co.st2) { (void)hipStreamSynchronize(co.st2); hpool().put_stream(co.st2); co.st2 = nullptr; }
        for (hipEvent_t *e : {&co.ev_up, &co.ev_next}) if (*e) { hpool().put_sync_event(*e); *e = nullptr; }
        for (int q = 0; q < 2; ++q) if (co.stc[q]) { (void)hipStreamSynchronize(co.stc[q]); hpool().put_stream(co.stc[q]); co.stc[q] = nullptr; }
    }
};

}  // namespace

// The runs of `seeds` on `device`, driven by the calling thread, up to max_in_flight of them in step on one stream, group after group.
// Device likelihoods: the built-in ones, a source handle, or the caller's DEVICE batch callback, whose function is called on this thread for
// the rows of the whole group (tg); a host callback belongs to its caller's thread.  Returns 0 or the first failing run's code.
extern "C" int pc_run_many(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nseeds, const int *seeds, int device,
                           int max_in_flight, pchip_result *results)
{
    for (int k = 0; k < nseeds; ++k) std::memset(&results[k], 0, sizeof(pchip_result));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { std::fprintf(stderr, "polychord_hip: no HIP device available -- this engine has no CPU path\n"); return PC_RC_DEVICE; }
    (void)hipSetDevice(device >= 0 ? device % ndev : 0);
    const int W = std::max(1, std::min(std::min(max_in_flight, nseeds), 64));
    int worst = 0;
    int done_here = 0;
    for (int base = 0; base < nseeds && !worst; base += done_here) {
        StepGroup g(s, like, prior, seeds + base, device, results + base, std::min(W, nseeds - base));
        try {
            g.pick_streams();
            g.set_up_runs();
            while (g.nlive > 0 && !g.worst) {
                g.compact_full();
                g.enqueue_round();
                g.await_round();
                g.finish_round();
                g.end_finished();
            }
        }
        catch (const EngineError &e) { std::fprintf(stderr, "polychord_hip: %s\n", e.msg.c_str()); (void)hipGetLastError(); if (!g.worst) g.worst = e.code; }
        catch (const std::bad_alloc &) { std::fprintf(stderr, "polychord_hip: out of host memory\n"); if (!g.worst) g.worst = PC_RC_MEMORY; }
        catch (const std::exception &e) { std::fprintf(stderr, "polychord_hip: %s\n", e.what()); if (!g.worst) g.worst = PC_RC_DEVICE; }      // (a thread that could not be started: nothing leaves through the C interface)
        g.join_endings();
        worst = g.worst;
        done_here = g.n;
    }      // (~StepGroup: release())
    return worst;
}
