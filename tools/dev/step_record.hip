// step_record.hip -- what the driver of the runs in step (pc_step.h: pc_run_many, StepGroup) asks of its engines, its streams and the device, recorded
// on the CPU.
//
// Includes pc_step.h with a scripted stand-in for Engine (the members the header's head comment lists, and no others), recorders for hpool(),
// sclasses(), cstreams(), the stream pickers, halloc / hfree and the HIP calls, and the real pc_fiber.h and pc_cohort.h (the cohort's launchers
// recorded as in cohort_record.hip).  A script says per run how many rounds it lasts, in which rounds its update may wait and how often it
// yields, where it compacts, and whether its set-up, begin, round_finish or ending fails.  No device, no kernel runs.  Built host-only
// (make -C polychordlite_amd/csrc step_record); tests/test_step_record.py compares the digests with those of the pc_run_many of the commit
// before the header (b330d9b).
//
//   step_record              one line per scenario: its name, the digest of its record, the number of lines
//   step_record --dump       the records themselves
//   step_record --gap        (not with STEP_PARENT) the event pool fails at its Nth request while the streams are picked, for every N: one line
//                            each -- N, the call's code, the streams and events not given back, the entries left in cstreams()
// PC_COHORT_SIDE=0, PC_COHORT_COPY_STREAMS=0, PC_COHORT_FIBERS=0: the same scenarios without the second stream, the copy streams, the fibers
// (a process each: the switches are read once); the scenarios' names say which.
// With -DSTEP_PARENT='"FILE"' (make step_record_parent STEP_PARENT='"FILE"': its own binary, step_record_parent) the same scenarios drive FILE
// instead: lines 2715-2999 of b330d9b's pc_engine.hip (its pc_run_many).
//
// What an ending thread does is written down per run and appended, in run order, where the driver gives the batch's event back (it has joined
// the thread just before): a record does not depend on the threads' timing.  The PC_DEBUG=5 report goes to stderr and is not recorded.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <vector>
#include <array>
#include <map>
#include <set>
#include <memory>
#include <atomic>
#include <mutex>
#include <thread>
#include <chrono>
#include <functional>
#include <algorithm>
#include <exception>
#include <initializer_list>
#include <new>
#include <ucontext.h>
#include <sys/mman.h>
#include <unistd.h>
#include "polychord_hip.h"
#include "pc_state.h"
#include "pc_launch.h"
#include "pc_plan.h"

enum { PC_RC_DEVICE = 2, PC_RC_MEMORY = 7, PC_RC_LIMIT = 8 };
struct EngineError { int code; std::string msg; };

struct Cohort;
namespace rec {
std::string text;                                   // the record of the scenario in progress (the driving thread's lines)
const std::thread::id driver = std::this_thread::get_id();
bool driving() { return std::this_thread::get_id() == driver; }
std::string run_lines[256];                         // what the ending threads did, by run
struct Batch { std::string lines; std::vector<int> runs; };
std::mutex batch_m; std::map<hipEvent_t, Batch> batches;      // by the batch's first event
thread_local Batch *my_batch = nullptr;
std::set<int> over;                                 // runs that are over and in no batch yet
Cohort *cur = nullptr;
pchip_result *results = nullptr;
const PcManyRec *dev_block = nullptr;
void line(const std::string &s) { text += s; text += '\n'; }
std::string num(long long v) { return std::to_string(v); }
std::string stream(hipStream_t q) { return q ? "s" + num(((long long)(uintptr_t)q - 0x1000) / 16) : "s-"; }
std::string event(hipEvent_t e) { return "e" + num(((long long)(uintptr_t)e - 0x100000) / 16); }
bool cohort_event(hipEvent_t e);
hipError_t event_record(hipEvent_t e, hipStream_t q)
{
    line("record " + event(e) + " on " + stream(q));
    if (!cohort_event(e) && !over.empty()) { std::lock_guard<std::mutex> g(batch_m); batches[e].runs.assign(over.begin(), over.end()); over.clear(); }
    return hipSuccess;
}
hipError_t stream_wait(hipStream_t q, hipEvent_t e) { line("wait " + event(e) + " on " + stream(q)); return hipSuccess; }
hipError_t event_sync(hipEvent_t e)
{
    if (driving()) { line("host waits " + event(e)); return hipSuccess; }
    if (!my_batch) { std::lock_guard<std::mutex> g(batch_m); my_batch = &batches.at(e); }
    my_batch->lines += "ending thread waits " + event(e) + "\n";
    return hipSuccess;
}
hipError_t stream_sync(hipStream_t q) { line("host waits " + stream(q)); return hipSuccess; }
hipError_t stream_query(hipStream_t q) { line("query " + stream(q)); return hipSuccess; }
hipError_t copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t q)
{
    std::memcpy(dst, src, bytes);
    if (kind == hipMemcpyHostToDevice) {
        dev_block = (const PcManyRec *)dst;
        const PcManyRec *r = (const PcManyRec *)src;
        std::string s = "upload on " + stream(q) + ":";
        for (size_t i = 0; i < bytes / sizeof(PcManyRec); ++i) s += " " + num(r[i].S.src_pad);
        line(s);
    } else line("rows in use " + num(*(const int *)src) + " to the host on " + stream(q));
    return hipSuccess;
}
int launch(const char *name, const PcState *S, const PcManyRec *d, int R, hipStream_t q)
{
    line(std::string("launch ") + name + (d ? " records " + num(d - dev_block) + "+" + num(R) : std::string()) + " run " + num(S ? S->src_pad : -1) + " on " + stream(q));
    return 0;
}
}

#define HIPCHK(x) (void)(x)
#define hipGetDeviceCount(p) (*(p) = 1, hipSuccess)
#define hipSetDevice(d) ((void)(d), hipSuccess)
#define hipGetDevice(p) (*(p) = 0, hipSuccess)
#define hipGetLastError() hipSuccess
#define hipEventRecord(e, q) rec::event_record(e, q)
#define hipStreamWaitEvent(q, e, flags) rec::stream_wait(q, e)
#define hipEventSynchronize(e) rec::event_sync(e)
#define hipStreamSynchronize(q) rec::stream_sync(q)
#define hipStreamQuery(q) rec::stream_query(q)
#define hipMemcpyAsync(dst, src, bytes, kind, q) rec::copy(dst, src, bytes, kind, q)

// ---- the services
template <class T> T *halloc(size_t n) { rec::line("host block of " + rec::num((long long)n)); return (T *)std::calloc(n ? n : 1, sizeof(T)); }
void hfree(void *p) { rec::line("host block freed"); std::free(p); }
template <class T> T *dalloc(size_t n) { rec::line("device block of " + rec::num((long long)n)); return (T *)std::calloc(n ? n : 1, sizeof(T)); }
template <class T> void dfree(T *&p) { rec::line("device block freed"); std::free((void *)p); p = nullptr; }
static void pc_copy_many(const std::vector<std::array<uintptr_t, 3>> &reqs, hipStream_t q) { rec::line("copies on " + rec::stream(q) + ": " + rec::num((long long)reqs.size())); }
struct Cache { long long cached = 0; };
static Cache &dcache() { static Cache c; return c; }
static Cache &hcache() { static Cache c; return c; }
static std::atomic<long long> g_dbg_miss_n[2], g_dbg_miss_ns[2], g_dbg_mk_stream_n{0}, g_dbg_mk_stream_ns{0};
static std::atomic<long long> g_dbg_compact_ns{0}, g_dbg_nursery_ns{0}, g_dbg_capacity_ns{0}, g_dbg_endb_ns{0}, g_dbg_destroy_ns{0}, g_dbg_evwait_ns{0}, g_dbg_d1{0}, g_dbg_d2{0};

// streams and events of the driving thread alone.  The pool keeps its streams from scenario to scenario, as a process does from call to call
struct HandlePool {
    std::vector<hipStream_t> streams; uintptr_t next_stream = 0x1000;
    std::vector<hipEvent_t> events; uintptr_t next_event = 0x100000;
    int streams_out = 0, events_out = 0, fail_event_in = 0;
    hipStream_t out(hipStream_t s, const char *how) { streams_out++; rec::line("stream " + rec::stream(s) + " " + how); return s; }
    hipStream_t get_stream()
    {
        if (!streams.empty()) { hipStream_t s = streams.front(); streams.erase(streams.begin()); return out(s, "from the pool"); }
        hipStream_t s = (hipStream_t)next_stream; next_stream += 16; return out(s, "made");
    }
    void put_stream(hipStream_t s) { streams_out--; rec::line("stream " + rec::stream(s) + " given back"); streams.push_back(s); }
    template <class Pred> hipStream_t take_stream_if(Pred pred)
    {
        for (size_t i = 0; i < streams.size(); ++i) if (pred(streams[i])) { hipStream_t s = streams[i]; streams.erase(streams.begin() + (long)i); return out(s, "picked from the pool"); }
        return nullptr;
    }
    hipEvent_t get_sync_event()
    {
        if (fail_event_in > 0 && --fail_event_in == 0) throw EngineError{PC_RC_DEVICE, "scripted: no event"};
        hipEvent_t e;
        if (!events.empty()) { e = events.back(); events.pop_back(); } else { e = (hipEvent_t)next_event; next_event += 16; }
        events_out++; rec::line("event " + rec::event(e) + " taken");
        return e;
    }
    void put_sync_event(hipEvent_t e)
    {
        events_out--; rec::line("event " + rec::event(e) + " given back"); events.push_back(e);
        std::lock_guard<std::mutex> g(rec::batch_m);
        auto it = rec::batches.find(e);
        if (it == rec::batches.end()) return;
        rec::text += it->second.lines;
        for (int r : it->second.runs) { rec::text += rec::run_lines[r]; rec::run_lines[r].clear(); }
        rec::batches.erase(it);
    }
};
HandlePool &hpool() { static HandlePool p; return p; }
// four hardware queues, dealt round robin as the streams are made
struct StreamClasses {
    std::map<void *, int> cls;
    int known(hipStream_t x) { auto it = cls.find((void *)x); return it == cls.end() ? -1 : it->second; }
    int classify(hipStream_t x)
    {
        if (known(x) < 0) { cls[(void *)x] = (int)((((uintptr_t)x - 0x1000) / 16) % 4); rec::line("class of " + rec::stream(x) + " tested: " + rec::num(cls[(void *)x])); }
        return cls[(void *)x];
    }
};
static StreamClasses &sclasses() { static StreamClasses c; return c; }
static std::string classes(const std::vector<int> &v) { std::string s; for (int c : v) s += " " + rec::num(c); return s; }
static hipStream_t stream_avoiding(std::vector<int> avoid, bool known_only = false)
{
    rec::line("a stream avoiding classes" + classes(avoid) + (known_only ? " (known ones only)" : ""));
    auto fits = [&](int c) { return c >= 0 && std::find(avoid.begin(), avoid.end(), c) == avoid.end(); };
    if (hipStream_t k = hpool().take_stream_if([&](hipStream_t x) { return fits(sclasses().known(x)); })) return k;
    hipStream_t s = hpool().get_stream();
    if (!known_only) (void)sclasses().classify(s);
    return s;
}
static hipStream_t stream_beside(std::initializer_list<hipStream_t> others, bool known_only = false)
{
    std::vector<int> avoid; std::string s = "a stream beside";
    for (hipStream_t o : others) if (o) { s += " " + rec::stream(o); const int c = known_only ? sclasses().known(o) : sclasses().classify(o); if (c >= 0) avoid.push_back(c); }
    rec::line(s);
    return stream_avoiding(avoid, known_only);
}
struct CohortStreams {
    std::mutex m;
    std::vector<std::pair<int, int>> used;      // (device, class; main streams' classes carry + 1000)
    std::vector<int> busy(int dev, bool mains_only = false)
    {
        std::vector<int> b;
        for (auto &u : used) if (u.first == dev && (!mains_only || u.second >= 1000)) b.push_back(u.second % 1000);
        rec::line(std::string("classes held on the device") + (mains_only ? " by main streams:" : ":") + classes(b));
        return b;
    }
    void take(int dev, int c, bool main_stream = false) { if (c >= 0) { used.emplace_back(dev, c + (main_stream ? 1000 : 0)); rec::line("class " + rec::num(c) + (main_stream ? " held for a main stream" : " held")); } }
    void give(int dev, int c, bool main_stream = false)
    {
        if (c < 0) return;
        const int v = c + (main_stream ? 1000 : 0);
        for (size_t i = 0; i < used.size(); ++i) if (used[i].first == dev && used[i].second == v) { used.erase(used.begin() + (long)i); rec::line("class " + rec::num(c) + " let go"); return; }
    }
};
static CohortStreams &cstreams() { static CohortStreams c; return c; }
struct CohortLease {
    int dev, cls_main = -1, cls_side = -1; bool held = false;
    explicit CohortLease(int d) : dev(d) {}
    void hold(int cm, int cs) { cls_main = cm; cls_side = cs; held = true; }
    void release() { if (!held) return; held = false; std::lock_guard<std::mutex> gq(cstreams().m); cstreams().give(dev, cls_main, true); cstreams().give(dev, cls_side); }
    ~CohortLease() { release(); }
};

#include "pc_fiber.h"
#include "pc_cohort.h"

bool rec::cohort_event(hipEvent_t e)
{
    if (!cur || !e) return false;
    if (e == cur->ev_up || e == cur->ev_next) return true;
    for (int k = 0; k < 4; ++k) if (e == cur->ev_seq[k]) return true;
    for (int k = 0; k < Cohort::RING; ++k) if (e == cur->ev[k] || e == cur->ev2[k]) return true;
    return false;
}

// ---- the launchers the cohort's table names: the launch, its records or its run, its stream
extern "C" {
void pc_launch_clean(const PcState *S, int, unsigned char *, int *, int *, double *, double *, unsigned *, unsigned long long *, int *, hipStream_t st) { rec::launch("clean", S, nullptr, 0, st); }
int pc_launch_clean_many(const PcManyRec *dR, int R, int, hipStream_t st) { return rec::launch("clean_many", nullptr, dR, R, st); }
void pc_launch_reset_thresholds(const PcState *S, hipStream_t st) { rec::launch("reset_thresholds", S, nullptr, 0, st); }
int pc_launch_reset_thresholds_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st) { return rec::launch("reset_thresholds_many", S, dR, R, st); }
int pc_launch_knn_cluster_batch_dev(const PcState *S, const int *, int, int, double *, int *, int *, int *, const int *, int, hipStream_t st) { return rec::launch("knn_cluster_batch_dev", S, nullptr, 0, st); }
int pc_launch_knn_cluster_batch_many(const PcState *S, const PcManyRec *dR, int R, int, int, int, hipStream_t st) { return rec::launch("knn_cluster_batch_many", S, dR, R, st); }
int pc_launch_knn_cluster_sub(const int *, int, int, const double *, const int *, int *, int *, int *, hipStream_t st) { return rec::launch("knn_cluster_sub", nullptr, nullptr, 0, st); }
int pc_launch_knn_cluster_sub_many(const PcManyRec *dR, int R, int, int, hipStream_t st) { return rec::launch("knn_cluster_sub_many", nullptr, dR, R, st); }
int pc_launch_nhats_part(const PcState *S, unsigned, int, int, hipStream_t st, int) { return rec::launch("nhats_part", S, nullptr, 0, st); }
int pc_launch_bases_t_many(const PcState *S, const PcManyRec *dR, int R, unsigned, int, hipStream_t st) { return rec::launch("bases_t_many", S, dR, R, st); }
int pc_launch_nhats(const PcState *S, unsigned, int, hipStream_t st) { return rec::launch("nhats", S, nullptr, 0, st); }
int pc_launch_nhats_many(const PcState *S, const PcManyRec *dR, int R, int, hipStream_t st) { return rec::launch("nhats_many", S, dR, R, st); }
int pc_launch_slice_t(const PcState *S, unsigned, int, hipStream_t st) { return rec::launch("slice_t", S, nullptr, 0, st); }
int pc_launch_slice_t_many(const PcState *S, const PcManyRec *dR, int R, unsigned, int, hipStream_t st) { return rec::launch("slice_t_many", S, dR, R, st); }
int pc_launch_slice(const PcState *S, unsigned, int, hipStream_t st) { return rec::launch("slice", S, nullptr, 0, st); }
int pc_launch_slice_fused(const PcState *S, unsigned, int, hipStream_t st) { return rec::launch("slice_fused", S, nullptr, 0, st); }
int pc_launch_slice_many(const PcState *S, const PcManyRec *dR, int R, int, int, hipStream_t st) { return rec::launch("slice_many", S, dR, R, st); }
int pc_launch_slice_step(const PcState *S, const PcManyRec *dR, int R, int, int, hipStream_t st) { return rec::launch("slice_step", S, dR, R, st); }
// (the tick stage of the device batch callback, CK_TICK: named by the cohort's table, in no scenario here)
void pc_launch_slice_tick_dev(const PcState *S, unsigned, int, void *, double *, int *, double *, const double *, const double *, const double *, int, const int *, hipStream_t st) { rec::launch("slice_tick_dev", S, nullptr, 0, st); }
int pc_launch_slice_tick_many(const PcManyRec *dR, int R, int, hipStream_t st) { return rec::launch("slice_tick_many", nullptr, dR, R, st); }
int pc_launch_sort_live(const PcState *S, hipStream_t st) { return rec::launch("sort_live", S, nullptr, 0, st); }
int pc_launch_sort_live_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st) { return rec::launch("sort_live_many", S, dR, R, st); }
void pc_launch_nn_lists(const PcState *S, int, int, hipStream_t st) { rec::launch("nn_lists", S, nullptr, 0, st); }
int pc_launch_nn_lists_many(const PcState *S, const PcManyRec *dR, int R, int, int, hipStream_t st) { return rec::launch("nn_lists_many", S, dR, R, st); }
int pc_launch_consume_par(const PcState *S, hipStream_t st) { return rec::launch("consume_par", S, nullptr, 0, st); }
int pc_launch_consume_par_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st) { return rec::launch("consume_par_many", S, dR, R, st); }
int pc_launch_consume_cl(const PcState *S, int, hipStream_t st) { return rec::launch("consume_cl", S, nullptr, 0, st); }
int pc_launch_consume_cl_many(const PcState *S, const PcManyRec *dR, int R, int, hipStream_t st) { return rec::launch("consume_cl_many", S, dR, R, st); }
void pc_launch_apply(const PcState *S, unsigned, int, hipStream_t st) { rec::launch("apply", S, nullptr, 0, st); }
int pc_launch_apply_many(const PcState *S, const PcManyRec *dR, int R, unsigned, int, hipStream_t st) { return rec::launch("apply_many", S, dR, R, st); }
void pc_launch_update_fused(const PcState *S, int, unsigned char *, int *, int *, double *, double *, unsigned *, unsigned long long *, double *, double *, int, hipStream_t st) { rec::launch("update_fused", S, nullptr, 0, st); }
int pc_launch_update_fused_many(const PcState *S, const PcManyRec *dR, int R, int, int, int, hipStream_t st) { return rec::launch("update_fused_many", S, dR, R, st); }
int pc_launch_final_par(const PcState *S, hipStream_t st) { return rec::launch("final_par", S, nullptr, 0, st); }
int pc_launch_final_par_many(const PcManyRec *dR, int R, hipStream_t st) { return rec::launch("final_par_many", nullptr, dR, R, st); }

void pchip_result_free(pchip_result *r)
{
    const int run = (int)(r - rec::results);
    const std::string s = "result of run " + rec::num(run) + " freed\n";
    if (rec::driving()) rec::text += s; else rec::run_lines[run] += s;
    std::memset(r, 0, sizeof(*r));
}
}

// ---- the scripted engine.  A run is named by its seed: the scenario's runs are seeds 0, 1, 2, ...
struct Script {
    int rounds = 3;                       // the run is over when this many rounds are finished
    unsigned wait_rounds = 0;             // bit r: finish_may_wait() in round r ...
    int yields = 0;                       // ... and round_finish() waits this often for the device there
    unsigned compact_rounds = 0;          // bit r: compact_wanted() before round r
    int setup_fails = 0, setup_how = 0;   // the first setup_fails set-ups throw: 1 no device memory, 2 another engine error, 3 no host memory
    int begin_rc = -1;                    // what begin() returns (-1: the rounds begin)
    int throw_round = -1, throw_after = 0;      // round_finish() throws in this round, after this many waits
    int rc_round = -1;                    // r_rc is set at the end of this round
    int end_b = 0;                        // what end_b() returns; -1: it throws
};
static std::vector<Script> script;
struct Engine {
    Cohort *co = nullptr; Fiber *fib = nullptr;
    int dev = 0; hipStream_t st_side = nullptr; int r_rc = 0; int rows = 0; int *d_total = &rows;
    int run = -1, round = 0, compacted = -1; Script sc; PcState S;
    void say(const std::string &what)
    {
        const std::string s = "run " + rec::num(run) + " " + what + "\n";
        if (rec::driving()) rec::text += s; else rec::run_lines[run] += s;
    }
    void setup(const pchip_settings &c, const pchip_like &, const pchip_prior &)
    {
        run = c.seed; sc = script[(size_t)run]; rec::cur = co; rows = 1000 + run;
        std::memset(&S, 0, sizeof S);
        S.src_pad = run; S.D = 8; S.nr = 16; S.N = 100; S.Ncap = 128; S.B = 32; S.pool = 1;
        if (run % 3 == 0) st_side = (hipStream_t)(uintptr_t)0x8;
        say("set up for device " + rec::num(c.device));
        if (script[(size_t)run].setup_fails > 0) {
            script[(size_t)run].setup_fails--;
            say("set-up fails");
            if (sc.setup_how == 3) throw std::bad_alloc();
            throw EngineError{sc.setup_how == 1 ? PC_RC_MEMORY : PC_RC_DEVICE, "scripted: set-up of run " + rec::num(run)};
        }
    }
    int begin() { say("begins: " + rec::num(sc.begin_rc)); return sc.begin_rc; }
    bool compact_wanted() const { return ((sc.compact_rounds >> round) & 1u) && compacted != round; }
    void compact_record() { say("writes its compaction down"); co->rec(rec_compact(S, nullptr, nullptr, d_total, nullptr, nullptr, nullptr, nullptr, rows)); }
    void compact_finish(int total) { say("compacted to " + rec::num(total) + " rows"); compacted = round; }
    bool round_enqueue() { say("writes round " + rec::num(round) + " down"); co->rec(rec_apply(S, (unsigned)round, 32)); return true; }
    bool round_ready() { say("ready"); return true; }
    bool finish_may_wait() const { return (sc.wait_rounds >> round) & 1u; }
    void sync_point()      // (as Engine::sync_point: inside a fiber yield, otherwise flush and wait)
    {
        if (fib) {
            fib->yield();
            if (fib->cancel) { say("cancelled"); throw FiberCancelled{}; }
            return;
        }
        co->flush();
        pc_wait_stream(co->st);
    }
    bool round_finish()
    {
        say("finishes round " + rec::num(round));
        const int waits = finish_may_wait() ? sc.yields : 0;
        for (int y = 0; y <= waits; ++y) {
            if (round == sc.throw_round && y == std::min(sc.throw_after, waits)) { say("throws"); throw EngineError{PC_RC_DEVICE, "scripted: update of run " + rec::num(run)}; }
            if (y == waits) break;
            const int r = run;
            co->rec(rec_reset(S)); co->pre_copies.push_back({1, 2, 3});
            co->post.push_back([r, y] { rec::line("run " + rec::num(r) + " reads back what wait " + rec::num(y) + " was for"); });
            sync_point();
            say("resumed");
        }
        if (round == sc.rc_round) { r_rc = PC_RC_LIMIT; say("fails with its own code"); rec::over.insert(run); return false; }
        if (++round >= sc.rounds) { rec::over.insert(run); return false; }
        return true;
    }
    void end_a(bool fused_final = false) { say(std::string("asks for its kill-off") + (fused_final ? " (fused)" : "")); co->rec(rec_final(S)); }
    void end_a2() { say("asks for its results"); }
    void end_wait_aside() { say("waits aside"); }
    int end_b(pchip_result *out)
    {
        say("makes its results: " + rec::num(sc.end_b));
        if (sc.end_b < 0) throw EngineError{PC_RC_DEVICE, "scripted: results of run " + rec::num(run)};
        out->ndead = run + 1;
        return sc.end_b;
    }
    // (what the cohort still has written down, where the driving thread destroys a run: the endings' threads run beside its rounds)
    void destroy(bool streams_idle = false)
    {
        say(std::string("destroyed") + (streams_idle ? " (streams idle)" : "") +
            (rec::driving() ? "; written down: " + rec::num((long long)co->pend.size()) + " records, " + rec::num((long long)(co->pre.size() + co->post.size())) + " closures, " + rec::num((long long)(co->pre_copies.size() + co->post_copies.size())) + " copies" : std::string()));
    }
};

// (what runs through the caller's device batch callback share, pc_tick.h: the scripted runs have no callback, the group's stays switched off)
struct TickGroup {
    bool on = false;
    static bool ticks(const pchip_like *like) { return like && like->kind == PCHIP_LIKE_CALLBACK; }
    void set_up(const std::vector<Engine *> &, const std::vector<char> &, int) {}
    void pack(hipStream_t) {}
    void answer() {}
    void leave(int) {}
    void drop() {}
    void release() {}
};

#ifdef STEP_PARENT
extern "C" {
#include STEP_PARENT
}
#else
#include "pc_step.h"
#endif

// ---- the scenarios
struct Scenario {
    std::vector<Script> runs; int max_in_flight = 64;
    std::vector<std::pair<int, int>> held;      // what other groups hold in cstreams() meanwhile
};
static bool dump = false;
static std::string variant;
static int drive(const Scenario &sc)
{
    script = sc.runs;
    const int n = (int)sc.runs.size();
    std::vector<int> seeds((size_t)n); for (int k = 0; k < n; ++k) seeds[(size_t)k] = k;
    std::vector<pchip_result> results((size_t)n);
    rec::results = results.data(); rec::over.clear(); rec::cur = nullptr;
    cstreams().used = sc.held;
    pchip_settings s; std::memset(&s, 0, sizeof s);
    pchip_like like; std::memset(&like, 0, sizeof like);
    pchip_prior prior; std::memset(&prior, 0, sizeof prior);
    const int rc = pc_run_many(&s, &like, &prior, n, seeds.data(), 0, sc.max_in_flight, results.data());
    std::string got;
    for (int k = 0; k < n; ++k) got += " " + rec::num(results[(size_t)k].ndead);
    rec::line("the call returns " + rec::num(rc) + "; results:" + got);
    rec::line("not given back: " + rec::num(hpool().streams_out) + " streams, " + rec::num(hpool().events_out) + " events, " + rec::num((long long)cstreams().used.size() - (long long)sc.held.size()) + " classes");
    return rc;
}
static void scenario(const std::string &name, const Scenario &sc)
{
    rec::text.clear();
    drive(sc);
    unsigned long long h = 1469598103934665603ull; long lines = 0;
    for (unsigned char ch : rec::text) { h ^= ch; h *= 1099511628211ull; lines += ch == '\n'; }
    std::printf("%s%s %016llx %ld\n", name.c_str(), variant.c_str(), h, lines);
    if (dump) std::printf("%s", rec::text.c_str());
}
// n runs that end in different rounds
static Scenario plain(int n) { Scenario sc; for (int k = 0; k < n; ++k) { Script r; r.rounds = 1 + (k * 7) % 5; sc.runs.push_back(r); } return sc; }
// ... whose updates wait in some rounds, one to three times, next to runs that finish at once
static Scenario waiting(int n)
{
    Scenario sc = plain(n);
    for (int k = 0; k < n; ++k) { Script &r = sc.runs[(size_t)k]; r.rounds += 2; if (k % 3 != 2) { r.wait_rounds = k % 2 ? 0x5u : 0xEu; r.yields = 1 + k % 3; } }
    return sc;
}

int main(int argc, char **argv)
{
    dump = argc > 1 && !std::strcmp(argv[1], "--dump");
    if (pc_env().cohort_side_off) variant += "_noside";
    if (pc_env().cohort_copy_streams_off) variant += "_nocopystreams";
    if (pc_env().cohort_fibers_off) variant += "_nofibers";
#ifndef STEP_PARENT
    if (argc > 1 && !std::strcmp(argv[1], "--gap")) {
        // how many events picking the streams asks for: the requests of a call whose only run fails at its set-up
        Scenario one = plain(1); one.runs[0].setup_fails = 1; one.runs[0].setup_how = 2;
        (void)drive(one);
        int asked = 0;
        for (size_t at = 0; (at = rec::text.find(" taken\n", at)) != std::string::npos; ++at) asked++;
        for (int nth = 1; nth <= asked; ++nth) {
            hpool().fail_event_in = nth;
            const int rc = drive(plain(3));
            std::printf("gap %d of %d: rc %d, not given back: %d streams, %d events, %d classes\n", nth, asked, rc, hpool().streams_out, hpool().events_out, (int)cstreams().used.size());
        }
        return 0;
    }
#endif
    for (int n : {1, 2, 5, 64}) scenario("group_" + std::to_string(n), plain(n));
    { Scenario sc = plain(7); sc.max_in_flight = 3; scenario("groups_3_3_1", sc); }
    { Scenario sc = plain(5); sc.max_in_flight = 2; scenario("groups_2_2_1", sc); }
    { Scenario sc = plain(3); sc.held = {{0, 1001}, {0, 2}}; scenario("device_busy", sc); }
    { Scenario sc = plain(3); sc.held = {{0, 1001}, {0, 2}, {0, 1003}, {0, 0}, {1, 1002}}; scenario("device_busy_four", sc); }
    { Scenario sc = plain(2); sc.held = {{0, 1000}, {0, 1001}, {0, 1002}, {0, 1003}}; scenario("device_busy_all_main", sc); }
    { Scenario sc = plain(5); for (int k = 0; k < 5; ++k) { sc.runs[(size_t)k].rounds = 4 + k % 2; sc.runs[(size_t)k].compact_rounds = k == 1 ? 0u : k == 3 ? 0xAu : (1u << k) | 1u; } scenario("compactions", sc); }
    scenario("waits_1", waiting(1));
    scenario("waits_6", waiting(6));
    scenario("waits_16", waiting(16));
    { Scenario sc = waiting(6); for (Script &r : sc.runs) r.compact_rounds = 0x4u; sc.max_in_flight = 4; scenario("waits_compactions_groups", sc); }
    // round_finish throws in the first, a middle and the last fiber while others are suspended; before its first wait, and with no wait at all
    for (int who : {0, 2, 4}) for (int after : {0, 1}) {
        Scenario sc = plain(5);
        for (Script &r : sc.runs) { r.rounds = 3; r.wait_rounds = 0x2u; r.yields = 2; }
        sc.runs[(size_t)who].throw_round = 1; sc.runs[(size_t)who].throw_after = after;
        scenario("update_throws_run_" + std::to_string(who) + "_after_" + std::to_string(after), sc);
    }
    { Scenario sc = waiting(5); sc.runs[2].throw_round = 1; scenario("update_throws_outside_a_fiber", sc); }
    { Scenario sc = waiting(4); sc.runs[1].rounds = 1; sc.runs[1].wait_rounds = 0; sc.runs[3].throw_round = 2; sc.runs[3].throw_after = 3; scenario("update_throws_with_an_ending_under_way", sc); }
    for (int how : {1, 2, 3}) { Scenario sc = plain(4); sc.runs[0].setup_fails = 1; sc.runs[0].setup_how = how; scenario("setup_fails_run_0_how_" + std::to_string(how), sc); }
    { Scenario sc = plain(6); sc.runs[3].setup_fails = 1; sc.runs[3].setup_how = 1; scenario("setup_no_memory_run_3", sc); }
    { Scenario sc = plain(7); sc.max_in_flight = 4; sc.runs[2].setup_fails = 1; sc.runs[2].setup_how = 1; sc.runs[5].setup_fails = 1; sc.runs[5].setup_how = 1; scenario("setup_no_memory_twice", sc); }
    for (int how : {2, 3}) { Scenario sc = plain(5); sc.runs[2].setup_fails = 1; sc.runs[2].setup_how = how; scenario("setup_fails_run_2_how_" + std::to_string(how), sc); }
    for (int rc : {0, 5}) { Scenario sc = plain(4); sc.runs[1].begin_rc = rc; scenario("begin_returns_" + std::to_string(rc), sc); }
    { Scenario sc = plain(5); for (Script &r : sc.runs) r.rounds = 4; sc.runs[2].rc_round = 1; scenario("a_run_fails_in_a_round", sc); }
    { Scenario sc = plain(5); sc.runs[0].rounds = 2; sc.runs[2].rounds = 2; sc.runs[2].rc_round = 1; scenario("a_run_fails_as_another_ends", sc); }
    for (int how : {7, -1}) { Scenario sc = plain(6); for (Script &r : sc.runs) r.rounds = 2; sc.runs[3].rounds = 4; sc.runs[1].end_b = how; scenario(std::string("results_fail_") + (how < 0 ? "thrown" : "code"), sc); }
    { Scenario sc = plain(12); for (Script &r : sc.runs) r.rounds = 2; scenario("ending_batch_of_12", sc); }
    return 0;
}
