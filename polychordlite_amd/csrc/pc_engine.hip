// pc_engine.hip -- host side of the MI355X nested-sampling engine.
//
// Replaces the administrator loop of NestedSampling (src/polychord/nested_sampling.F90:15-510) and
// the MPI live-point farm (mpi_utils.F90:322-600): the host only enqueues kernels and reads one
// small control block per round; every point, every evidence accumulator and every decision lives
// on the device.  One round = [K0 directions | K1 slice chains] (when the nursery is empty)
// + [K2 consume | K3 apply] + (on an update) [clean phantoms | covariance + Cholesky].
#include "pc_state.h"
#include "pc_resume.h"
#include "pc_prior_table.h"
#include "pc_launch.h"
#include "pc_plan.h"       // which kernels a run, a nursery, a contraction and an update take; the developer switches of the environment (pc_env)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <cstdint>
#include <new>
#include <cmath>
#include <vector>
#include <memory>
#include <string>
#include <chrono>
#include <algorithm>
#include <map>
#include <unordered_map>
#include <atomic>
#include <mutex>
#include <thread>
#include <functional>
#include <exception>
#include <ucontext.h>
#include <array>
#include <sys/mman.h>
#include <unistd.h>

// Fatal conditions unwind to the C ABI entry points (pchip_run_hooks, pchip_slice_chains), which release the run's
// resources, print the message and return the code: the reference's convention is message + `stop 1`
// (abort.F90:19-29), and the process-level half of it belongs to the caller of the C ABI (polychord_c_interface exits;
// a language binding raises) -- an engine inside somebody's interpreter must not take the process down itself.
enum { PC_RC_SETTINGS = 1, PC_RC_DEVICE = 2, PC_RC_NDIMS = 3, PC_RC_LDS = 4, PC_RC_STOPPED = 5, PC_RC_RESUME = 6, PC_RC_MEMORY = 7, PC_RC_LIMIT = 8 };
struct EngineError {
    int code; std::string msg;
};
[[noreturn]] static void engine_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
[[noreturn]] static void engine_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); std::vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    throw EngineError{code, buf};
}
static std::atomic<int> g_cap_clusters{128}, g_cap_phantoms{0};   // initial capacities (both grow on demand); tests shrink them
static std::atomic<int> g_inject_fault{0};           // polychord_hip_set_option("inject_fault", k): tests of the error paths, one-shot
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    engine_fail(PC_RC_DEVICE, "HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// polychord_hip_set_batch_callback / polychord_hip_request_stop are process-level calls of the C ABI (no run handle, like
// the reference's setup_loglikelihood state).  A run takes its OWN copy of the batch callback when it is set up and owns
// its OWN stop flag; a stop request raises the flag of every run in flight at that moment (the registry below) and of no
// later one -- runs on other threads (pchip_run_repeats) neither lose a request nor inherit a stale one.
static std::mutex g_cb_mutex;
static polychord_batch_fn g_batch_fn = nullptr;     // polychord_hip_set_batch_callback
static void *g_batch_user = nullptr;
static polychord_device_batch_fn g_dbatch_fn = nullptr;     // polychord_hip_set_device_batch_callback
static void *g_dbatch_user = nullptr;
static std::mutex g_run_mutex;
static std::vector<std::atomic<int> *> g_run_stop;  // stop flags of the runs in flight
extern "C" double polychord_hip_keyed_uniform(unsigned seed, unsigned dom, unsigned shi, unsigned slo, unsigned idx);

namespace {

static std::atomic<long long> g_dbg_miss_n[2], g_dbg_miss_ns[2], g_dbg_mk_stream_n{0}, g_dbg_mk_stream_ns{0};      // (PC_DEBUG=5: trips to the driver -- device / pinned blocks, streams)
#include "pc_blocks.h"      // BlockCache and dalloc / dfree / halloc / hfree; RunBlocks: the ledger of the blocks a run holds

// streams and events are pooled for the same reason (creation / destruction synchronise with the driver)
struct HandlePool {
    std::mutex m;
    std::vector<std::pair<int, hipStream_t>> streams;
    std::vector<std::pair<int, hipEvent_t>> events;
    hipStream_t get_stream()
    {
        int dev = 0; (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(m);
            for (size_t i = 0; i < streams.size(); ++i)
                if (streams[i].first == dev) { hipStream_t s = streams[i].second; streams.erase(streams.begin() + i); return s; }
        }
        const auto q0 = std::chrono::steady_clock::now();
        hipStream_t s; HIPCHK(hipStreamCreate(&s));
        g_dbg_mk_stream_n++; g_dbg_mk_stream_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - q0).count();
        return s;
    }
    void put_stream(hipStream_t s) { int dev = 0; (void)hipGetDevice(&dev); std::lock_guard<std::mutex> g(m); streams.push_back({dev, s}); }
    template <class Pred> hipStream_t take_stream_if(Pred pred)          // a pooled stream of this device the predicate accepts, or null
    {
        int dev = 0; (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> g(m);
        for (size_t i = 0; i < streams.size(); ++i)
            if (streams[i].first == dev && pred(streams[i].second)) { hipStream_t s = streams[i].second; streams.erase(streams.begin() + i); return s; }
        return nullptr;
    }
    hipEvent_t get_event()
    {
        int dev = 0; (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(m);
            for (size_t i = events.size(); i-- > 0;)
                if (events[i].first == dev) { hipEvent_t e = events[i].second; events.erase(events.begin() + i); return e; }
        }
        hipEvent_t e; HIPCHK(hipEventCreate(&e)); return e;
    }
    void put_event(hipEvent_t e) { int dev = 0; (void)hipGetDevice(&dev); std::lock_guard<std::mutex> g(m); events.push_back({dev, e}); }
    // events that only order streams (no timestamps: a cheaper record)
    std::vector<std::pair<int, hipEvent_t>> sync_events;
    hipEvent_t get_sync_event()
    {
        int dev = 0; (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(m);
            for (size_t i = sync_events.size(); i-- > 0;)
                if (sync_events[i].first == dev) { hipEvent_t e = sync_events[i].second; sync_events.erase(sync_events.begin() + i); return e; }
        }
        hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return e;
    }
    void put_sync_event(hipEvent_t e) { int dev = 0; (void)hipGetDevice(&dev); std::lock_guard<std::mutex> g(m); sync_events.push_back({dev, e}); }
};
HandlePool &hpool() { static HandlePool *p = new HandlePool; return *p; }

// A second stream is worth something only if the device runs it NEXT TO the first: the runtime deals streams onto a few hardware
// queues (GPU_MAX_HW_QUEUES, four by default), and two streams of one queue take turns -- after a sweep of sixty-four runs in
// step the pool held dozens of streams, and a single run that drew two of one queue was 2.3 ms (16 %) slower.  So a side stream
// is tried against its main stream once (two 40-us spinning kernels: together or one after the other?) and the verdict kept.
// ---- the small copies of runs in step, many at a time.  An update with clustering reads a dozen small arrays back and sends a dozen
// down (add_cluster: counts, evidences, the cross-volume matrix, labels); as hipMemcpyAsync calls that was 49 000 copies for sixteen
// 10-D Rastrigin runs (round 4) -- ~6 us of the driving thread each, and on the stream one after the other, ~4 us each, in front of
// every shared wait.  Pinned host memory is mapped into the device's address space (hipHostMalloc), so ONE kernel makes up to PC_COPY_N
// of them, either way, a workgroup per piece of at most 4 KB: its arguments are the (source, destination, bytes) of the pieces.
#define PC_COPY_N 96
#define PC_COPY_PIECE 4096u
struct PcCopyBatch { const void *src[PC_COPY_N]; void *dst[PC_COPY_N]; unsigned bytes[PC_COPY_N]; };
__global__ __launch_bounds__(256) void k_copy_batch(PcCopyBatch b)
{
    const int i = blockIdx.x;
    const unsigned n = b.bytes[i];
    const char *s = (const char *)b.src[i]; char *d = (char *)b.dst[i];
    if ((((uintptr_t)s | (uintptr_t)d) & 7u) == 0u) {
        const unsigned n8 = n >> 3;
        for (unsigned k = threadIdx.x; k < n8; k += 256) ((unsigned long long *)d)[k] = ((const unsigned long long *)s)[k];
        for (unsigned k = (n8 << 3) + threadIdx.x; k < n; k += 256) d[k] = s[k];
    } else for (unsigned k = threadIdx.x; k < n; k += 256) d[k] = s[k];
}
static void pc_copy_many(const std::vector<std::array<uintptr_t, 3>> &reqs, hipStream_t q)      // {dst, src, bytes}
{
    PcCopyBatch b; int n = 0;
    auto go = [&] { if (n) { hipLaunchKernelGGL(k_copy_batch, dim3(n), dim3(256), 0, q, b); n = 0; } };
    for (const auto &r : reqs) {
        size_t left = r[2]; uintptr_t d = r[0], s = r[1];
        while (left) {
            const unsigned c = (unsigned)std::min<size_t>(left, PC_COPY_PIECE);
            b.dst[n] = (void *)d; b.src[n] = (const void *)s; b.bytes[n] = c; ++n;
            d += c; s += c; left -= c;
            if (n == PC_COPY_N) go();
        }
    }
    go();
}

__global__ void k_engine_spin(long long ticks) { const long long t0 = wall_clock64(); while (wall_clock64() - t0 < ticks) {} }
static bool streams_overlap_test(hipStream_t a, hipStream_t b)
{
    auto both = [&] {
        (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_engine_spin, dim3(1), dim3(64), 0, a, 10000LL);              // 100 us of the 100 MHz clock
        hipLaunchKernelGGL(k_engine_spin, dim3(1), dim3(64), 0, b, 10000LL);
        (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    static std::atomic<bool> warmed{false};
    if (!warmed.exchange(true)) (void)both();                // (the kernel's first launch loads its code)
    const double two = std::min(both(), both());
    if (pc_env().debug == 5) std::fprintf(stderr, "polychord_hip dbg streams %p %p: both %.1f us\n", (void *)a, (void *)b, two * 1e6);
    return two < 170e-6;                                    // side by side: ~120 us (one spin and the launches); in turn: ~225 us
}
// streams that take turns are streams of one hardware queue: every stream is put into its class once (one test against a
// member of each class known so far), and two streams run side by side when their classes differ
struct StreamClasses {
    std::mutex mm;
    std::map<void *, int> cls;
    std::vector<hipStream_t> reps;
    int known(hipStream_t x) { std::lock_guard<std::mutex> g(mm); auto it = cls.find((void *)x); return it == cls.end() ? -1 : it->second; }
    int classify(hipStream_t x)
    {
        std::lock_guard<std::mutex> g(mm);
        auto it = cls.find((void *)x);
        if (it != cls.end()) return it->second;
        int c = -1;
        for (size_t r = 0; r < reps.size() && c < 0; ++r) if (!streams_overlap_test(reps[r], x)) c = (int)r;
        if (c < 0) { c = (int)reps.size(); reps.push_back(x); }
        cls[(void *)x] = c;
        return c;
    }
};
static StreamClasses &sclasses() { static StreamClasses *p = new StreamClasses; return *p; }
// a pooled (or new) stream that runs next to all of `others` (null entries ignored): one whose class is known first, then the
// pool's unknown ones, classed as they come; the ones found wanting go back to the pool
static hipStream_t stream_avoiding(std::vector<int> avoid, bool known_only = false);
static hipStream_t stream_beside(std::initializer_list<hipStream_t> others, bool known_only = false)
{
    if (pc_env().side_pick_off) return hpool().get_stream();
    std::vector<int> avoid;
    for (hipStream_t o : others) if (o) { const int c = known_only ? sclasses().known(o) : sclasses().classify(o); if (c >= 0) avoid.push_back(c); }
    return stream_avoiding(avoid, known_only);
}
// ... next to every stream of the hardware-queue classes in `avoid`.  known_only: the device is at work (another scheduler group's runs):
// a class test now -- two spin kernels timed side by side -- would say "one queue" for whatever pair it is given, and the wrong class would
// stay with the stream; only streams classed earlier (pc_prepare_streams) are looked at, the best of them taken
static hipStream_t stream_avoiding(std::vector<int> avoid, bool known_only)
{
    auto fits = [&](int c) { return c >= 0 && std::find(avoid.begin(), avoid.end(), c) == avoid.end(); };
    if (hipStream_t k = hpool().take_stream_if([&](hipStream_t x) { return fits(sclasses().known(x)); })) return k;
    if (known_only) {
        if (hipStream_t k = hpool().take_stream_if([&](hipStream_t x) { return sclasses().known(x) >= 0; })) return k;
        return hpool().get_stream();
    }
    std::vector<hipStream_t> tried;
    hipStream_t pick = nullptr;
    for (int k = 0; k < 8 && !pick; ++k) {
        hipStream_t c = hpool().take_stream_if([&](hipStream_t x) { return sclasses().known(x) < 0; });
        const bool dbg = pc_env().debug == 5;
        const auto q0 = std::chrono::steady_clock::now();
        const bool made = !c;
        if (!c) { HIPCHK(hipStreamCreate(&c)); }
        const auto q1 = std::chrono::steady_clock::now();
        const int cc = sclasses().classify(c);
        if (dbg) std::fprintf(stderr, "polychord_hip dbg stream_beside: try %d, %s stream %p (%.2f ms), class %d (%.2f ms), avoid %d\n", k, made ? "new" : "pooled", (void *)c, std::chrono::duration<double>(q1 - q0).count() * 1e3, cc, std::chrono::duration<double>(std::chrono::steady_clock::now() - q1).count() * 1e3, avoid.empty() ? -1 : avoid[0]);
        if (fits(cc)) pick = c; else tried.push_back(c);
    }
    if (!pick) { pick = tried.back(); tried.pop_back(); }   // (none: any will do)
    for (hipStream_t t : tried) hpool().put_stream(t);
    return pick;
}
static hipStream_t side_stream_for(hipStream_t main_st) { return stream_beside({main_st}); }
// The hardware-queue classes the scheduler groups at work on a device have taken for their main and side streams.  Two groups side by
// side (clustered runs: pchip_run_repeats) each picked their streams from the pool on their own, and now and then both main streams sat
// on ONE hardware queue: their kernels took turns, sixteen twin-Gaussian runs 590 ms instead of 370 -- which of the two a process got
// depended on what it had done before (a merge, a torch.cuda.synchronize: whatever moved the pool's order).  A group now takes streams
// of classes no other group of its device holds, while there are any.
struct CohortStreams {
    std::mutex m;
    std::vector<std::pair<int, int>> used;      // (device, class; main streams' classes carry + 1000)
    std::vector<int> busy(int dev, bool mains_only = false)
    {
        std::vector<int> b;
        for (auto &u : used) if (u.first == dev && (!mains_only || u.second >= 1000)) b.push_back(u.second % 1000);
        return b;
    }
    void take(int dev, int c, bool main_stream = false) { if (c >= 0) used.emplace_back(dev, c + (main_stream ? 1000 : 0)); }
    // (the exact entry that was taken: by class alone a group handing back its SIDE stream's class could erase another group's MAIN entry of the
    //  same class, and busy(dev, mains_only) then misreports which hardware queues hold main streams)
    void give(int dev, int c, bool main_stream = false)
    {
        if (c < 0) return;
        const int v = c + (main_stream ? 1000 : 0);
        for (size_t i = 0; i < used.size(); ++i) if (used[i].first == dev && used[i].second == v) { used.erase(used.begin() + (long)i); return; }
    }
};
static CohortStreams &cstreams() { static CohortStreams *p = new CohortStreams; return *p; }
// what a scheduler group holds of the table above, given back when the group is done -- or when anything between the take and that point throws
struct CohortLease {
    int dev, cls_main = -1, cls_side = -1; bool held = false;
    explicit CohortLease(int d) : dev(d) {}
    void hold(int cm, int cs) { cls_main = cm; cls_side = cs; held = true; }      // (the caller holds cstreams().m: take() has just been called)
    void release() { if (!held) return; held = false; std::lock_guard<std::mutex> gq(cstreams().m); cstreams().give(dev, cls_main, true); cstreams().give(dev, cls_side); }
    ~CohortLease() { release(); }
};
// called before several scheduler groups start on a device, while it is idle: the pool gets at least `want` streams whose hardware-queue
// class is known (a group takes four: main, side, two for copies), so that no group has to class a stream while another group's kernels run
extern "C" void pc_prepare_streams(int dev, int want)
{
    if (hipSetDevice(dev) != hipSuccess) return;
    (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> gq(cstreams().m);
    std::vector<hipStream_t> have;
    while (hipStream_t k = hpool().take_stream_if([](hipStream_t x) { return sclasses().known(x) >= 0; })) have.push_back(k);
    for (int tries = 0; (int)have.size() < want && tries < 4 * want; ++tries) {
        hipStream_t c = hpool().take_stream_if([](hipStream_t x) { return sclasses().known(x) < 0; });
        if (!c && hipStreamCreate(&c) != hipSuccess) break;
        (void)sclasses().classify(c);
        have.push_back(c);
    }
    for (hipStream_t k : have) hpool().put_stream(k);
}
std::atomic<int> g_active_runs{0};         // runs in flight in this process (pchip_run_repeats: one thread each)
std::atomic<int> g_active_dev[64];         // ... per HIP device (zero-initialised: static storage)

struct Timing { double t_gen = 0, t_loop = 0, t_final = 0, t_total = 0; long rounds = 0, updates = 0, batches = 0, compactions = 0; };

// HIP-event stopwatch per kernel class, on the engine's own stream (bench.py's roofline numbers)
enum { KT_NHATS = 0, KT_SLICE, KT_CONSUME, KT_APPLY, KT_CLEAN, KT_COV, KT_SIDE /* bases drawn ahead on the side stream */, KT_N };
struct KTimer {
    bool on = false;
    unsigned mask = 0xFFFFFFFFu;            // kernel classes that are timed
    unsigned stride = 1; unsigned seen[KT_N] = {0};   // ... every stride-th launch of a class (an event pair costs the stream ~6 us)
    hipStream_t st = nullptr;
    std::vector<hipEvent_t> pool; size_t used = 0;
    struct Span { int k; hipEvent_t a, b; bool side; };
    std::vector<Span> open;
    double total_ms[KT_N] = {0}; long launches[KT_N] = {0};
    hipEvent_t get() { if (used == pool.size()) pool.push_back(hpool().get_event()); return pool[used++]; }
    hipEvent_t begin(int k) { if (!on || !((mask >> k) & 1u) || (seen[k]++ % stride) != 0 || open.size() >= MAX_OPEN) return nullptr; hipEvent_t e = get(); HIPCHK(hipEventRecord(e, st)); return e; }
    void end(int k, hipEvent_t a) { if (!on || !a) return; hipEvent_t e = get(); HIPCHK(hipEventRecord(e, st)); open.push_back({k, a, e, false}); }
    // the same around a launch on another stream of the run (the bases drawn ahead): collect() waits for that span's end itself
    hipEvent_t begin_on(int k, hipStream_t s2) { if (!on || !((mask >> k) & 1u) || (seen[k]++ % stride) != 0 || open.size() >= MAX_OPEN) return nullptr; hipEvent_t e = get(); HIPCHK(hipEventRecord(e, s2)); return e; }
    void end_on(int k, hipEvent_t a, hipStream_t s2) { if (!on || !a) return; hipEvent_t e = get(); HIPCHK(hipEventRecord(e, s2)); open.push_back({k, a, e, true}); }
    // Call after a stream synchronisation.  A round no longer synchronises, so the spans pile up between the moments that
    // do (an update with host work, a compaction, a growth, the end of the run); beyond MAX_OPEN open spans launches go
    // untimed (k_launches counts the timed ones) instead of creating events without bound.
    static constexpr size_t MAX_OPEN = 8192;
    void collect() {
        if (!on) return;
        for (auto &sp : open) { float ms = 0; if (sp.side) HIPCHK(hipEventSynchronize(sp.b)); HIPCHK(hipEventElapsedTime(&ms, sp.a, sp.b)); total_ms[sp.k] += ms; launches[sp.k]++; }
        open.clear(); used = 0;
    }
    void destroy() { for (auto e : pool) hpool().put_event(e); pool.clear(); }
};

// host copy of the device's counter RNG (pc_dev.h), used when the host evaluates the likelihood
static void h_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4])
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
static double h_uniform(uint32_t k0, uint32_t k1, uint32_t dom, uint32_t shi, uint32_t slo, uint32_t idx)
{
    uint32_t o[4];
    h_philox(idx >> 1, slo, shi, dom, k0, k1, o);
    const uint64_t w = (idx & 1u) ? (((uint64_t)o[2] << 32) | o[3]) : (((uint64_t)o[0] << 32) | o[1]);
    return ((double)(w >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// ---- the runs of a device in step (pchip_run_repeats with a built-in likelihood): a kernel launched on N streams at once costs
//      every one of them tens of microseconds on this device (tools/dev/ubench_queues.hip: an empty kernel 3 us alone, 36 us
//      each with sixteen streams busy; at most ~8 kernels at a time whatever the number of hardware queues), so the runs share
//      ONE stream and go round by round together: what each engine would launch in a phase of the round it writes down here, and
//      every kernel of the phase is launched ONCE for all of them (blockIdx.y = run, PcManyRec).  The same kernels' bodies on
//      the same states: the numbers of a run do not know whether it ran alone.
#include "pc_fiber.h"       // Fiber: a run's host work that has to wait for the device in the middle, as a fiber of the driving thread; pc_wait_stream

#include "pc_cohort.h"      // Cohort: the launches of the runs in step, written down and made once for all of them (the table of stages)

#include "pc_split.h"       // ClusterUpdate: the host's half of a clustering update -- first pass, recursion level by level, add_cluster

// adds its lifetime to one of the counters below
struct DbgSpan {
    std::atomic<long long> &ns; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~DbgSpan() { ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};
static std::atomic<long long> g_dbg_compact_ns{0}, g_dbg_nursery_ns{0}, g_dbg_capacity_ns{0}, g_dbg_endb_ns{0}, g_dbg_destroy_ns{0}, g_dbg_evwait_ns{0}, g_dbg_d1{0}, g_dbg_d2{0};      // (PC_DEBUG=5: where round_enqueue's time goes)
struct Engine {
    Cohort *co = nullptr;               // not null: this run goes in step with others of its device, on their common stream
    Fiber *fib = nullptr;               // not null: this call runs as a fiber of the thread that drives the runs in step (waits are shared)
    pchip_settings cfg{};
    std::atomic<int> stop{0};                   // polychord_hip_request_stop reached this run
    polychord_batch_fn batch_fn = nullptr; void *batch_user = nullptr;     // the batch callback registered when the run was set up
    // host-callback mode (device proposes, host evaluates): pc_callback.hip
    polychord_loglike_fn cb_like = nullptr; polychord_prior_fn cb_prior = nullptr;
    bool callback_mode = false;
    void *d_cs = nullptr; double *d_x0s = nullptr, *d_prop = nullptr;
    int *d_decks = nullptr;
    // pinned host side of the propose / evaluate exchange: the kernel stores proposals and need flags here directly; the
    // answers (logL | theta | phi of every chain, one block) go back in one copy
    double *hp_prop = nullptr, *hp_ans = nullptr, *d_ans = nullptr; int *hp_need = nullptr;
    long long cb_evals = 0; long cb_ticks = 0;
    // the device batch callback registered when the run was set up (it wins over batch_fn): the parked proposals of a round packed into
    // dense device blocks, the answers read at the chains' ranks (pc_park.hip) -- the host reads *hp_count a round and nothing else
    polychord_device_batch_fn dbatch_fn = nullptr; void *dbatch_user = nullptr;
    bool dev_batch = false; int db_flags = 0;              // db_flags bit 0: the engine evaluates the prior (box or table) on the blocks
    PcState S_pri{};                                       // ... the state k_prior_transform reads for it (nDims, the prior, the table's mask)
    // A batched quadratic form behind the likelihood (pchip_source_create_quad_batch): the run is a device-batch run whose callback is the
    // library's own evaluator, quad_batch_call -- three launches for the rows of a tick (pc_launch_quad_batch).  qb_nres > 0 says so; S_qb is
    // the source state the two run-time kernels are launched with (the handle, its block on this device), qb_R / qb_part the scratch for
    // qb_rows rows: a longer block is evaluated slab by slab (a row's bits do not depend on the cut)
    int qb_nres = 0; PcState S_qb{}; double *qb_R = nullptr, *qb_part = nullptr; long qb_rows = 0;
    static double quad_batch_no_host(double *, int, double *, int) { return -1.7976931348623157e308; }      // (callback mode's scalar function: never reached on the device batch path)
    static int quad_batch_call(void *user, int n, int, int, const double *, double *theta, double *phi, double *logL, int, void *stream)
    {
        Engine *e = (Engine *)user;
        const int nDer = e->S_qb.nDer;
        for (long at = 0; at < n; at += e->qb_rows) {
            const int m = (int)std::min<long>(e->qb_rows, n - at);
            if (pc_launch_quad_batch(&e->S_qb, e->qb_nres, m, theta + (size_t)at * e->S_qb.D, logL + at, phi + (size_t)at * nDer, e->qb_R, e->qb_part, (hipStream_t)stream))
                engine_fail(PC_RC_SETTINGS, "the batched quadratic form could not be evaluated: %.400s", pc_rtc_error() ? pc_rtc_error() : "no such launch");
        }
        return 0;
    }
    double *db_cube = nullptr, *db_theta = nullptr, *db_phi = nullptr, *db_logL = nullptr;
    int *db_rank = nullptr, *db_count = nullptr, *hp_count = nullptr, *hp_count_dev = nullptr;
    // ... in step with other runs (TickGroup, pc_tick.h): the four blocks are the group's ONE block, a tick is written down and the run yields;
    // tick_want says where its flags, proposals and ranks are, tick_count comes back with the rows the pack found for it
    bool tick_shared = false, tick_asked = false; PcParkRun tick_want{}; int tick_count = 0;
    std::vector<int> cb_idx; std::vector<double> cb_c, cb_t, cb_p, cb_l;   // batch callback scratch
    // host mirror of the dead points for the dumper hook (nested_sampling.F90:546-590)
    polychord_dumper_fn dumper = nullptr;
    pchip_update_fn on_update = nullptr; void *hook_user = nullptr;
    long ndiscarded = 0;                        // prior samples rejected while generating the live points
    bool resume_static = true; unsigned resume_batch0 = 0;
    bool nph_stale = false;                     // h_ctl->nphantom is the count before the last clean (an upper bound)
    std::vector<double> hm_dead, hm_logw; int hm_ndead = 0;
    std::vector<unsigned> hm_cuid;              // cluster uid every dead point died in
    // boost_posterior: phantoms removed by a clean that were kept as posterior samples (run_time_info.f90:857-870)
    std::vector<double> pp_rows, pp_logpost; std::vector<unsigned> pp_cuid; std::vector<unsigned long long> pp_uid; int nd_last_update = 0;
    // cluster genealogy: child uid, parent uid, log of the evidence fraction the child received (add_cluster)
    std::vector<unsigned> split_child, split_parent; std::vector<double> split_logfrac;
    std::vector<double> h_lo, h_hi;
    PcState S{};
    RunBlocks blocks;                         // every device and pinned block the run holds: allocated through it, released from it (destroy)
    hipStream_t st = nullptr;
    hipStream_t st_copy = nullptr;            // dead rows leave for the host while the run goes on
    bool st_copy_shared = false;              // ... one of the cohort's two (not this run's to give back)
    hipStream_t st_side = nullptr;            // the orthonormal bases of the next nursery, while this one is consumed
    hipEvent_t ev_main = nullptr;
    // ring of bases drawn ahead on the side stream: nursery b's live in raw_buf[b % raw_depth]
    static constexpr int RAW_RING = 4;
    struct RawSlot { hipEvent_t ready = nullptr, consumed = nullptr; unsigned batch = 0; int B = 0; bool valid = false, waited = false, used = false; int co_seq = 0; };
    RawSlot ring[RAW_RING];
    int raw_depth = 2;
    double *h_dead = nullptr; size_t h_dead_cap = 0, h_dead_copied = 0;
    // a run on its own in pool mode: the row kernel's launch carries the update's flag pass (settings.ablate bit 17: not).  What the round in
    // flight was launched with, for do_update:
    bool r_flagged = false; int r_flag_nph = 0; unsigned char *r_flag_keep = nullptr; int *r_flag_blk = nullptr;
    PcCtl *h_ctl = nullptr;       // pinned mirror
    PcCtl *h_note = nullptr;      // pinned, device-visible: the contraction kernels publish the control block here (pc_publish_ctl)
    unsigned note_seq = 0;
    hipEvent_t ev_apply = nullptr;
    double *raw_buf[RAW_RING] = {nullptr, nullptr, nullptr, nullptr};
    // alternate phantom buffers + scratch for the update step
    double *ph2 = nullptr, *phL2 = nullptr; unsigned *phC2 = nullptr; unsigned long long *phU2 = nullptr;
    unsigned char *keep = nullptr; int *blk = nullptr, *d_total = nullptr;
    double *psum = nullptr, *mean = nullptr, *pcov = nullptr; int *pcnt = nullptr, *count = nullptr;
    size_t cov_chunks_cap = 0;
    double *upd_part = nullptr, *upd_shift = nullptr; size_t upd_part_cap = 0;   // fused update (pc_update.hip)
    PcPriorTable ptab; bool have_ptab = false;      // prior.kind == PCHIP_PRIOR_TABLE: checked copy (the host function of callback mode; what went to the device)
    double *d_lo = nullptr, *d_hi = nullptr, *d_invcovT = nullptr, *d_mean = nullptr, *d_src = nullptr;
    double *d_dynL = nullptr; int *d_dynN = nullptr; double *d_logn = nullptr;
    ClusterUpdate<Engine> clus{*this};         // the host's half of a clustering update and its scratch on the device (pc_split.h)
    Engine() = default; Engine(const Engine &) = delete; Engine &operator=(const Engine &) = delete;     // (clus refers to this Engine)
    std::vector<int> sub_dims; int *c_subdims = nullptr;     // sub-dimension clustering: the run's coordinates (settings.sub_cluster_dims), on the device
    long nsplits = 0; int ncluster_peak = 1;
    bool src_terms = false;                    // a source likelihood in the terms form (pchip_source_create_terms)
    long path[PCHIP_PATH_COUNT] = {};          // launches per kernel variant (pchip_result.path): counted where the choice is made
    Cohort::Note step_note;                    // in step: what Cohort::flush made of this run's sampling records (PCHIP_PATH_SLICE_STEP; a launch nobody took)
    Timing tm;
    KTimer kt;
    int B = 0, dev = 0;
    bool cb_auto_batch = false; int B_small = 1; double cb_eval_seconds = -1.0;   // host callbacks: chains per nursery chosen from the measured cost of a call
    long long nlike_g[PC_MAX_GRADE] = {0};      // RTI%nlike per grade (grade 1 includes the prior samples)
    std::vector<int> h_nlike_g;                 // [B][PC_MAX_GRADE] of the batch in the nursery

    void alloc_phantom_side(int Pcap)
    {
        ph2 = blocks.dev<double>((size_t)Pcap * S.nT); phL2 = blocks.dev<double>(Pcap); phC2 = blocks.dev<unsigned>(Pcap);
        phU2 = blocks.dev<unsigned long long>(Pcap); keep = blocks.dev<unsigned char>(Pcap); blk = blocks.dev<int>((Pcap + 255) / 256 + 1);
    }

    // a small table of the set-up on its way to the device: through a pinned block of the cache, in stream order (a blocking copy
    // from pageable memory was 0.1 ms as a rule and 4 ... 11 ms now and then -- one run in eight or so -- while the driver pinned
    // the vector's pages); the blocks go back at the teardown
    void upload(void *dst, const void *src, size_t bytes)
    {
        void *h = blocks.pin<char>(bytes);
        std::memcpy(h, src, bytes);
        HIPCHK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st));
    }
    void setup(const pchip_settings &c, const pchip_like &like_in, const pchip_prior &prior)
    {
        cfg = c;
        { std::lock_guard<std::mutex> g(g_cb_mutex); batch_fn = g_batch_fn; batch_user = g_batch_user; dbatch_fn = g_dbatch_fn; dbatch_user = g_dbatch_user; }
        // a batched quadratic form: to everything below a callback likelihood behind a device batch callback -- the library's own, whatever
        // the caller has registered
        pchip_like like = like_in;
        if (const char *why = pc_quad_batch_refusal("pchip_run", &like_in, &prior, &qb_nres)) { pc_abi_set_last_error(why); engine_fail(PC_RC_SETTINGS, "%s", why); }
        if (qb_nres > 0) { like.kind = PC_LIKE_CALLBACK; like.fn = quad_batch_no_host; batch_fn = nullptr; batch_user = nullptr; dbatch_fn = quad_batch_call; dbatch_user = this; }
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
            engine_fail(PC_RC_DEVICE, "no HIP device available -- this engine has no CPU path");
        }
        dev = c.device >= 0 ? c.device % ndev : 0;
        HIPCHK(hipSetDevice(dev));
        st = co ? co->st : hpool().get_stream();
        st_copy = (co && co->stc[0]) ? co->stc[(co->n_stc++) & 1] : (co ? hpool().get_stream() : stream_beside({st}));      // (a run on its own: its copies on another hardware queue than its kernels)
        st_copy_shared = co && co->stc[0];
        kt.on = c.profile != 0 && !co; kt.st = st;      // (in step with other runs the launches are made elsewhere: nothing of its own to time)
        kt.mask = (c.profile == 1) ? 0xFFFFFFFFu : (((unsigned)c.profile >> 1) & 0x7Fu);   // 1: every class; else bit k+1 = class k
        kt.stride = std::max(1u, ((unsigned)c.profile >> 8) & 0xFFu);                       // bits 8..15: time every n-th launch of a class
        const int D = c.nDims, nDer = c.nDerived;
        S.D = D; S.nDer = nDer; S.nT = 2 * D + nDer + 2; S.nr = c.num_repeats; S.N = c.nlive;
        // grades (chordal_sampling.f90:119-130): bases per grade, first direction and first deviate of each
        S.ngrade = 1; S.g_off[0] = 0; S.g_nr[0] = c.num_repeats;
        for (int g = 1; g < PC_MAX_GRADE; ++g) { S.g_off[g] = 0; S.g_nr[g] = 0; }
        if (c.nGrade > 1 && c.grade_dims && c.grade_repeats) {
            if (c.nGrade > PC_MAX_GRADE) engine_fail(PC_RC_SETTINGS, "at most %d parameter grades", PC_MAX_GRADE);
            S.ngrade = c.nGrade;
            int off = 0, tot = 0;
            for (int g = 0; g < c.nGrade; ++g) {
                if (c.grade_dims[g] < 1 || c.grade_repeats[g] < 1) engine_fail(PC_RC_SETTINGS, "every grade needs at least one parameter and one repeat");
                S.g_off[g] = off; off += c.grade_dims[g]; S.g_nr[g] = c.grade_repeats[g]; tot += c.grade_repeats[g];
            }
            if (off != D) engine_fail(PC_RC_SETTINGS, "grade_dims must sum to nDims");
            S.nr = tot; cfg.num_repeats = tot;
        }
        S.nb_total = 0; S.n_dev = 0;
        for (int g = 0, col = 0; g < PC_MAX_GRADE; ++g) {
            const int Dg = D - S.g_off[g];
            S.g_nb[g] = g < S.ngrade ? (S.g_nr[g] + Dg - 1) / Dg : 0;
            S.g_col0[g] = col; S.g_e0[g] = (int)S.n_dev;
            col += S.g_nr[g]; S.nb_total += S.g_nb[g]; S.n_dev += (unsigned)S.g_nb[g] * Dg * Dg;
        }
        // sub-dimension clustering: the list is checked whether or not the run clusters (a bad list is a bad setting either way)
        sub_dims.clear();
        if (c.n_sub_cluster < 0 || (c.n_sub_cluster > 0 && !c.sub_cluster_dims)) engine_fail(PC_RC_SETTINGS, "n_sub_cluster = %d without a list of coordinates", c.n_sub_cluster);
        for (int k = 0; k < c.n_sub_cluster; ++k) {
            const int d = c.sub_cluster_dims[k];
            if (d < 0 || d >= D) engine_fail(PC_RC_SETTINGS, "sub-clustering coordinate %d out of range (nDims = %d; the indices are 0-based)", d, D);
            if (std::find(sub_dims.begin(), sub_dims.end(), d) != sub_dims.end()) engine_fail(PC_RC_SETTINGS, "sub-clustering coordinate %d given twice", d);
            sub_dims.push_back(d);
        }
        S.ch_nlike_g = nullptr;
        std::memset(nlike_g, 0, sizeof(nlike_g));
        S.p0 = D; S.d0 = 2 * D; S.b0 = 2 * D + nDer; S.l0 = S.b0 + 1;
        int nmax = c.nlive;
        for (int i = 0; i < c.n_nlives; ++i) nmax = std::max(nmax, c.nlives[i]);
        const int nprior = c.nprior <= 0 ? c.nlive : c.nprior;
        S.Ncap = std::max(nmax, nprior);
        B = c.batch > 0 ? c.batch : std::max(1, std::min(1024, c.nlive / 2));
        // (the contraction kernels stamp the nursery position into 16 bits of the host mirror, pc_state.h pc_note: never truncate silently)
        if (B > 65535) engine_fail(PC_RC_LIMIT, "batch = %d chains per nursery: at most 65535", B);
        if (c.sequential_rng) B = 1;
        // Host callbacks: every chain of a nursery is seeded from one snapshot, so about B / (2 nlive) of the evaluations
        // are spent on spawns that fail -- cheap for a compiled likelihood (then the round trips per nursery dominate and
        // many chains per nursery pay: nlive / 2), dear for an expensive one (nlive / 4, at most 64).  Which one this is
        // is measured while the live points are generated; buffers are sized for the larger choice.
        cb_auto_batch = c.batch <= 0 && !c.sequential_rng && qb_nres == 0 && (like.kind == PC_LIKE_CALLBACK || (prior.kind != 1 && prior.kind != PCHIP_PRIOR_TABLE && prior.kind != PCHIP_PRIOR_SOURCE));
        if (cb_auto_batch) B_small = std::max(1, std::min(64, c.nlive / 4));
        S.B = B;
        S.maxc = c.do_clustering ? std::max(2, g_cap_clusters.load()) : 4;
        S.maxc_dead = 4096;
        S.Pcap = (int)std::min<long long>(2000000000LL / S.nT, 4LL * S.nr * S.Ncap + 4LL * B * S.nr + 1024);
        if (g_cap_phantoms.load() > 0) S.Pcap = std::max(g_cap_phantoms.load(), B * S.nr + 16);
        S.Dcap = 64 * S.Ncap + 4 * B + 1024;
        S.k0 = (uint32_t)c.seed; S.k1 = 0x504F4C59u;
        S.logzero = c.logzero; S.use_prec = c.precision_criterion > 0;
        S.log_prec = S.use_prec ? std::log(c.precision_criterion) : 0.0;
        S.log_cf = std::log(c.compression_factor);
        S.max_ndead = c.max_ndead; S.nfail = c.nfail <= 0 ? c.nlive : c.nfail;
        S.seed_override = 0; S.ablate = c.ablate; S.seq_mode = c.sequential_rng ? 1 : 0;
        S.epoch_discard = c.epoch_discard ? 1 : 0;
        if (S.seq_mode) { cfg.batch = 1; cfg.force_general = 1; }
        // dynamic nlive tables
        S.n_nlives = c.n_nlives;
        if (c.n_nlives > 0) {
            d_dynL = blocks.dev<double>(c.n_nlives); d_dynN = blocks.dev<int>(c.n_nlives);
            upload(d_dynL, c.loglikes, sizeof(double) * c.n_nlives);
            upload(d_dynN, c.nlives, sizeof(int) * c.n_nlives);
        }
        S.dyn_loglikes = d_dynL; S.dyn_nlives = d_dynN;
        // likelihood / prior
        S.like.kind = like.kind; S.like.mu = like.mu; S.like.sigma = like.sigma; S.like.logdetcov = like.logdetcov;
        S.like.norm = -(double)D * (std::log(like.sigma > 0 ? like.sigma : 1.0) + PC_LOG_TWO_PI / 2.0);
        S.like.inv_sigma = like.sigma > 0 ? 1.0 / like.sigma : 1.0;
        S.like.log_vn = 0.5 * D * std::log(3.14159265358979323846) - std::lgamma(1.0 + D / 2.0);
        S.like.invcov = nullptr; S.like.mean = nullptr;
        S.src_id = 0; S.src_pad = 0; S.src_data = nullptr; S.src_ndata = 0;
        if (like.kind == PC_LIKE_SOURCE) {         // a user's device source (pc_rtc.hip): its data block goes up with the run
            PcSourceForm f;
            const auto hold = pc_rtc_source_hold(like.source, &f);      // (kept until the block is in the pinned staging buffer: upload)
            if (!hold) engine_fail(PC_RC_SETTINGS, "device source handle %d does not exist", like.source);
            if (nDer > PC_SRC_MAX_DERIVED) engine_fail(PC_RC_SETTINGS, "a device source likelihood writes at most %d derived parameters, not %d", PC_SRC_MAX_DERIVED, nDer);
            if (prior.kind != 1 && prior.kind != PCHIP_PRIOR_TABLE && prior.kind != PCHIP_PRIOR_SOURCE)
                engine_fail(PC_RC_SETTINGS, "a device source likelihood needs a device prior (the uniform box, a table or its own source prior: prior.kind 1, 2 or 3), not a host-callback prior");
            if (prior.kind == PCHIP_PRIOR_SOURCE && !f.has_prior)
                engine_fail(PC_RC_SETTINGS, "prior.kind = 3 (source prior): device source handle %d defines no pchip_prior_param -- make it with pchip_source_create_prior", like.source);
            S.src_id = like.source;
            src_terms = f.nterms > 0;
            // (a quadratic form: its precision matrix goes up behind the user's data, in the same block -- the kernels find it at src_data + src_ndata)
            if (!hold->empty()) { d_src = blocks.dev<double>(hold->size()); upload(d_src, hold->data(), sizeof(double) * hold->size()); S.src_data = d_src; S.src_ndata = f.ndata; }
        }
        if (qb_nres > 0) {      // the batched quadratic form: its block (the matrix behind the user's data) goes up like any handle's, for the evaluator's state
            PcSourceForm f;
            const auto hold = pc_rtc_source_hold(like_in.source, &f);
            if (!hold) engine_fail(PC_RC_SETTINGS, "device source handle %d does not exist", like_in.source);
            if (nDer > PC_SRC_MAX_DERIVED) engine_fail(PC_RC_SETTINGS, "a device source likelihood writes at most %d derived parameters, not %d", PC_SRC_MAX_DERIVED, nDer);
            d_src = blocks.dev<double>(hold->size()); upload(d_src, hold->data(), sizeof(double) * hold->size());
            std::memset(&S_qb, 0, sizeof(S_qb));
            S_qb.D = D; S_qb.nDer = nDer; S_qb.like.kind = PC_LIKE_SOURCE; S_qb.src_id = like_in.source; S_qb.src_data = d_src; S_qb.src_ndata = f.ndata;
        }
        // a source prior is the handle's own function, inside the sampling kernels: there is no host function for callback mode to call
        if (prior.kind == PCHIP_PRIOR_SOURCE && like.kind != PC_LIKE_SOURCE)
            engine_fail(PC_RC_SETTINGS, "prior.kind = 3 (source prior) needs a device source likelihood of the same handle (like.kind = %d is none): a prior-only source is not supported", like.kind);
        if (prior.kind == PCHIP_PRIOR_SOURCE && c.feedback >= 1) { std::printf("prior source evaluated on the device, inside the sampling kernels (pchip_prior_param of source handle %d)\n", like.source); std::fflush(stdout); }
        if (like.kind == PC_LIKE_CORR_GAUSSIAN) {
            std::vector<double> T((size_t)D * D);
            for (int a = 0; a < D; ++a) for (int b = 0; b < D; ++b) T[(size_t)b * D + a] = like.invcov[(size_t)a * D + b];
            d_invcovT = blocks.dev<double>((size_t)D * D); d_mean = blocks.dev<double>(D);
            upload(d_invcovT, T.data(), sizeof(double) * D * D);
            upload(d_mean, like.mean, sizeof(double) * D);
            S.like.invcov = d_invcovT; S.like.mean = d_mean;
        }
        // A prior table: checked once.  With a callback likelihood it serves as the host prior function; with a device likelihood
        // it goes up once -- S.prior.lo carries the per-parameter doubles, S.prior.hi the per-parameter integers, S.src_pad the mask of
        // the types present (pc_table_theta, pc_sample.hip: PcState keeps its size and every kernel of a box run its arguments) --
        // unless it IS a box (all uniform, identity order): then the run is the box run, bit for bit.
        have_ptab = false;
        int prior_kind = prior.kind;
        std::vector<double> box_lo, box_hi;
        const double *p_lo = prior.lo, *p_hi = prior.hi;
        if (prior.kind == PCHIP_PRIOR_TABLE) {
            const std::string err = pc_prior_table_build(D, prior.table, prior.hyper, ptab);
            if (!err.empty()) { pc_abi_set_last_error(err.c_str()); engine_fail(PC_RC_SETTINGS, "%s", err.c_str()); }
            have_ptab = true;
            if (ptab.is_box && like.kind != PC_LIKE_CALLBACK) {
                box_lo.resize(D); box_hi.resize(D);
                for (int i = 0; i < D; ++i) { box_lo[i] = ptab.e[i].par[0]; box_hi[i] = ptab.e[i].par[1]; }
                prior_kind = 1; p_lo = box_lo.data(); p_hi = box_hi.data();
            }
        } else if (prior.kind != 0 && prior.kind != 1 && prior.kind != PCHIP_PRIOR_SOURCE) engine_fail(PC_RC_SETTINGS, "prior.kind = %d: 0 (callback), 1 (uniform box), 2 (table) or 3 (source)", prior.kind);
        callback_mode = (like.kind == PC_LIKE_CALLBACK) || (prior_kind != 1 && prior_kind != PCHIP_PRIOR_TABLE && prior_kind != PCHIP_PRIOR_SOURCE);
        if (callback_mode) {
            cb_like = like.fn; cb_prior = prior.kind == PCHIP_PRIOR_TABLE ? nullptr : prior.fn;      // (a table is its own host function: host_eval)
            if (!cb_like) engine_fail(PC_RC_SETTINGS, "callback mode needs a loglikelihood function pointer");
        }
        S.prior.kind = callback_mode ? (prior_kind == PCHIP_PRIOR_TABLE ? 0 : prior_kind) : prior_kind; S.prior.lo = nullptr; S.prior.hi = nullptr;
        if (prior_kind == 1 && p_lo && p_hi) {
            d_lo = blocks.dev<double>(D); d_hi = blocks.dev<double>(D);
            upload(d_lo, p_lo, sizeof(double) * D);
            upload(d_hi, p_hi, sizeof(double) * D);
            S.prior.lo = d_lo; S.prior.hi = d_hi;
        }
        if (S.prior.kind == PCHIP_PRIOR_TABLE) {
            const std::vector<double> tp = ptab.dev_par(); const std::vector<int> ti = ptab.dev_int();
            d_lo = blocks.dev<double>(tp.size()); d_hi = blocks.dev<double>((ti.size() + 1) / 2);
            upload(d_lo, tp.data(), sizeof(double) * tp.size());
            upload(d_hi, ti.data(), sizeof(int) * ti.size());
            S.prior.lo = d_lo; S.prior.hi = d_hi; S.src_pad = (int)ptab.mask;
        }
        // The device batch callback: a callback likelihood only.  Under the box or a table the engine transforms the packed cubes itself
        // (flags bit 0), by k_prior_transform on a state of its own -- the sampling state of callback mode carries no table.
        dev_batch = dbatch_fn != nullptr && like.kind == PC_LIKE_CALLBACK;
        db_flags = 0;
        if (dev_batch) {
            std::memset(&S_pri, 0, sizeof(S_pri));
            S_pri.D = D;
            if (prior_kind == 1) { S_pri.prior.kind = 1; S_pri.prior.lo = d_lo; S_pri.prior.hi = d_hi; db_flags = 1; }
            else if (prior_kind == PCHIP_PRIOR_TABLE) {
                const std::vector<double> tp = ptab.dev_par(); const std::vector<int> ti = ptab.dev_int();
                d_lo = blocks.dev<double>(tp.size()); d_hi = blocks.dev<double>((ti.size() + 1) / 2);
                upload(d_lo, tp.data(), sizeof(double) * tp.size());
                upload(d_hi, ti.data(), sizeof(int) * ti.size());
                S_pri.prior.kind = PCHIP_PRIOR_TABLE; S_pri.prior.lo = d_lo; S_pri.prior.hi = d_hi; S_pri.src_pad = (int)ptab.mask; db_flags = 1;
            }
            if (db_flags && D > 256) engine_fail(PC_RC_NDIMS, "the device batch callback under a device prior (box or table): nDims <= 256, not %d", D);
            if (qb_nres > 0 && !db_flags) engine_fail(PC_RC_SETTINGS, "a batched quadratic form needs the uniform box or a prior table (prior.kind 1 or 2), not prior.kind = %d", prior.kind);
            if (c.feedback >= 1) {
                if (qb_nres > 0) std::printf("likelihood: batched quadratic form of %d residuals (device source handle %d), evaluated in batches on the matrix cores, three launches a round; prior on the device\n", qb_nres, like_in.source);
                else std::printf("likelihood evaluated on the device in batches through the caller's device callback; prior %s\n", db_flags ? "on the device" : "by the callback");
                std::fflush(stdout);
            }
        }
        // state arrays
        const int Ncap = S.Ncap, maxc = S.maxc, nT = S.nT, nr = S.nr;
        S.live = blocks.dev<double>((size_t)Ncap * nT); S.live_logL = blocks.dev<double>(Ncap);
        S.live_cluster = blocks.dev<int>(Ncap); S.live_pos = blocks.dev<int>(Ncap); S.live_entry = blocks.dev<double>(Ncap);
        S.cl_list = blocks.dev<int>((size_t)maxc * Ncap); S.cl_n = blocks.dev<int>(maxc);
        S.logZp = blocks.dev<double>(maxc); S.logXp = blocks.dev<double>(maxc); S.logZXp = blocks.dev<double>(maxc);
        S.logZp2 = blocks.dev<double>(maxc); S.logZpXp = blocks.dev<double>(maxc); S.logLp = blocks.dev<double>(maxc);
        S.XpXq = blocks.dev<double>(2 * (size_t)maxc * maxc); S.imin_slot = blocks.dev<int>(maxc);      // (the second half: k_consume_clp's copy of the matrix in linear space, made anew by every pass)
        S.lse_ref = blocks.dev<double>(maxc); S.lse_sum = blocks.dev<double>(maxc); S.death_thr = blocks.dev<double>(maxc);
        S.cl_uid = blocks.dev<unsigned>(maxc);
        S.chol = blocks.dev<double>((size_t)maxc * D * D); S.cov = blocks.dev<double>((size_t)maxc * D * D);
        S.logZp_dead = blocks.dev<double>(S.maxc_dead); S.logZp2_dead = blocks.dev<double>(S.maxc_dead); S.cl_uid_dead = blocks.dev<unsigned>(S.maxc_dead);
        S.phantom = blocks.dev<double>((size_t)S.Pcap * nT); S.ph_logL = blocks.dev<double>(S.Pcap);
        S.ph_cuid = blocks.dev<unsigned>(S.Pcap); S.ph_uid = blocks.dev<unsigned long long>(S.Pcap);
        alloc_phantom_side(S.Pcap);
        S.dead = blocks.dev<double>((size_t)S.Dcap * nT); S.dead_logw = blocks.dev<double>(S.Dcap);
        S.dead_postX = blocks.dev<double>(S.Dcap); S.dead_postZ = blocks.dev<double>(S.Dcap); S.dead_cuid = blocks.dev<unsigned>(S.Dcap);
        S.dead_entry = blocks.dev<double>(S.Dcap);
        S.babies = blocks.dev<double>((size_t)B * nr * nT); S.baby_logL = blocks.dev<double>((size_t)B * nr); S.baby_logL_T = blocks.dev<double>((size_t)B * nr);
        S.ch_cluster = blocks.dev<int>(B); S.ch_epoch = blocks.dev<int>(B); S.ch_nlike = blocks.dev<int>(B); S.ch_seed_slot = blocks.dev<int>(B);
        S.ch_contour = blocks.dev<double>(B);
        if (S.ngrade > 1) { S.ch_nlike_g = blocks.dev<int>((size_t)B * PC_MAX_GRADE); h_nlike_g.assign((size_t)B * PC_MAX_GRADE, 0); }
        {   // log k for the evidence update of the serial kernel
            std::vector<double> ln((size_t)Ncap + 4);
            ln[0] = -PC_HUGE;
            for (int k = 1; k < Ncap + 4; ++k) ln[k] = std::log((double)k);
            d_logn = blocks.dev<double>(ln.size());
            upload(d_logn, ln.data(), sizeof(double) * ln.size());
            S.logn = d_logn;
        }
        S.nn_list = nullptr; S.nn_slot_owner = nullptr; S.nn_chain_slot = nullptr; S.nn_pts = nullptr; S.nn_code = nullptr; S.nn_valid = 0;
        if (c.do_clustering) {      // candidate lists of the nearest-cluster search (k_nn_lists)
            S.nn_list = blocks.dev<int>((size_t)B * nr * PC_NN_K); S.nn_slot_owner = blocks.dev<int>(Ncap); S.nn_chain_slot = blocks.dev<int>(B);
            S.nn_pts = blocks.dev<double>((size_t)(Ncap + B) * D); S.nn_code = blocks.dev<int>((size_t)2 * Ncap + B + 64);      // (codes of the candidates, then the ranks of the live points and their number: k_sort_live)
            if (!sub_dims.empty()) { c_subdims = blocks.dev<int>(sub_dims.size()); upload(c_subdims, sub_dims.data(), sizeof(int) * sub_dims.size()); }
        }
        S.nhat = blocks.dev<double>((size_t)B * nr * D); S.nhat_w = blocks.dev<double>((size_t)B * nr);
        const bool ms_pre = S.like.kind == PC_LIKE_CORR_GAUSSIAN && D > 64 && D <= 128 && S.ngrade <= 1 && !S.seq_mode && !(S.ablate & PC_ABL_FUNCTOR) && !pc_env().ms_pre_off && S.prior.kind < PCHIP_PRIOR_TABLE;
        S.nhat_Ms = ms_pre ? blocks.dev<double>((size_t)B * nr * D) : nullptr;
        S.ch_My = ms_pre ? blocks.dev<double>((size_t)B * D) : nullptr;
        const bool split_off = pc_env().nhats_split_off;
        // 64 < nDims <= 128, one grade: k_nhats_q<32, 1> leaves a basis register-major, 32 x 512 doubles
        const bool split_q = D > 64 && D <= 128 && S.ngrade <= 1 && !S.seq_mode && !split_off && !callback_mode;
        // 24 < nDims <= 64, one grade (round 5): k_nhats_q<8 / 16, 1> leaves a basis thread by thread, 16 HV^2 doubles
        const bool split_m = D > 24 && D <= 64 && S.ngrade <= 1 && !S.seq_mode && !split_off && !callback_mode;
        const size_t raw_n = split_q ? (size_t)B * S.nb_total * 32 * 512 : split_m ? (size_t)B * S.nb_total * (D <= 32 ? 1024 : 4096) : (size_t)B * S.nb_total * D * D + (size_t)B * 33 + 8;      // (+ the chains' deck records, 66 ints each: pc_deck_record, pc_seed.h)
        S.nhat_raw = ((D <= 24 && !S.seq_mode && !split_off) || split_q || split_m) ? blocks.dev<double>(raw_n)
                   : (D > 128 ? blocks.dev<double>((size_t)B * S.nb_total * D * 256) : nullptr);   // k_nhats_big keeps its bases there
        // split launch: two buffers, so that the bases of nursery b + 1 can be drawn at any time while nursery b's are read
        // (nDims > 64: the bases cost more than the rest of a nursery's round -- they are drawn up to three nurseries ahead,
        //  through the updates as well)
        // (nDims <= 24: three -- the bases of nursery b + 2 are drawn under nursery b's contraction.  With two, nursery b + 1's were drawn
        //  there and k_slice(b + 1) waited for them across streams: kernel 39 us + ~10 us for the event to cross, a path as long as
        //  contraction + row copies + the host's look at the stamp, which is why enqueueing k_slice ahead changed nothing)
        raw_depth = split_q ? RAW_RING : std::min((int)RAW_RING, pc_env().raw_depth);
        raw_buf[0] = S.nhat_raw;
        for (int r = 1; r < raw_depth; ++r) raw_buf[r] = ((D <= 24 || split_q || split_m) && S.nhat_raw) ? blocks.dev<double>(raw_n) : nullptr;
        S.plan = blocks.dev<PcPlan>(B); S.slot_src = blocks.dev<int>(Ncap); S.slot_step = blocks.dev<int>(Ncap); S.slot_dead = blocks.dev<int>(Ncap); HIPCHK(hipMemsetAsync(S.slot_dead, 0xFF, sizeof(int) * Ncap, st)); S.defer_update = 0; S.sort_slot = blocks.dev<int>(Ncap + 64); S.sort_key = blocks.dev<unsigned long long>(Ncap + 64);
        S.ctl = blocks.dev<PcCtl>(1);
        d_total = blocks.dev<int>(PC_UPD_CTR_INTS); HIPCHK(hipMemsetAsync(d_total, 0, sizeof(int) * PC_UPD_CTR_INTS, st));      // (the count, and the update chain's tickets: dalloc recycles memory as it is)
        if (callback_mode) {
            d_cs = (void *)blocks.dev<char>(pc_chain_state_size() * B); d_x0s = blocks.dev<double>((size_t)B * D); d_prop = blocks.dev<double>((size_t)B * D);
            const size_t nans = (size_t)B * (1 + D + std::max(1, nDer));
            if (dev_batch) {      // dense blocks for a nursery's round or the prior samples of the live points, whichever is more rows
                const size_t cap = (size_t)std::max(B, nprior);
                db_cube = blocks.dev<double>(cap * D); db_theta = blocks.dev<double>(cap * D); db_phi = blocks.dev<double>(cap * std::max(1, nDer));
                db_logL = blocks.dev<double>(cap); db_rank = blocks.dev<int>(B); db_count = blocks.dev<int>(1);
                if (qb_nres > 0) {      // the evaluator's scratch: residuals [rows][ldr], partial sums [rows][ncb]
                    qb_rows = pc_quad_mm_rows((long)std::min<size_t>(cap, PC_QUAD_BATCH_SLAB));
                    qb_R = blocks.dev<double>((size_t)qb_rows * pc_quad_mm_ldr(qb_nres)); qb_part = blocks.dev<double>((size_t)qb_rows * pc_quad_mm_ncb(qb_nres));
                }
                hp_count = blocks.pin<int>(1); *hp_count = 0;
                { void *dp = nullptr; HIPCHK(hipHostGetDevicePointer(&dp, hp_count, 0)); hp_count_dev = (int *)dp; }
                HIPCHK(hipMemsetAsync(db_rank, 0xFF, sizeof(int) * B, st));
                HIPCHK(hipMemsetAsync(db_phi, 0, sizeof(double) * cap * std::max(1, nDer), st));
                d_decks = blocks.dev<int>((size_t)B * nr);
            } else {
            d_ans = blocks.dev<double>(nans);
            d_decks = blocks.dev<int>((size_t)B * nr);
            hp_prop = blocks.pin<double>((size_t)B * D); hp_ans = blocks.pin<double>(nans); hp_need = blocks.pin<int>(B);
            std::memset(hp_ans, 0, sizeof(double) * nans); std::memset(hp_need, 0, sizeof(int) * B);
            }
            HIPCHK(hipMemset(d_cs, 0, pc_chain_state_size() * B));
        }
        h_ctl = blocks.pin<PcCtl>(1);
        h_note = blocks.pin<PcCtl>(1);                    // (hipHostMalloc memory is mapped and coherent: the device stores straight into it)
        std::memset(h_note, 0, sizeof(PcCtl)); note_seq = 0;
        { void *dp = nullptr; HIPCHK(hipHostGetDevicePointer(&dp, h_note, 0)); S.ctl_host = (PcCtl *)dp; }
        S.notify_seq = 0;
        // per-cluster initial values and the control block (initialise_run_time_info, run_time_info.f90:164-206)
        pc_launch_init_state(&S, c.logzero, st);
        PcCtl c0{};
        c0.status = PC_ST_RUNNING; c0.ncluster = 1; c0.logZ = c.logzero; c0.logZ2 = c.logzero;
        c0.logX_last_update = 0.0; c0.next_cluster_uid = 1; c0.live_logZ = c.logzero;
        *h_ctl = c0;
    }

    void grade_counts(long *o)
    {   // grade 1 carries the prior samples (generate.F90:294); with one grade it is simply nlike
        for (int g = 0; g < PC_MAX_GRADE; ++g) o[g] = 0;
        if (S.ngrade <= 1) { o[0] = (long)h_ctl->nlike; return; }
        long rest = 0;
        for (int g = 1; g < S.ngrade; ++g) { o[g] = (long)nlike_g[g]; rest += o[g]; }
        o[0] = (long)h_ctl->nlike - rest;
    }

    // per-grade likelihood counts (RTI%nlike, nested_sampling.F90:307): the chains the last segment consumed
    void tally_grades()
    {
        if (S.ngrade <= 1) return;
        for (int w = h_ctl->seg_lo; w <= h_ctl->seg_hi; ++w)
            for (int g = 0; g < PC_MAX_GRADE; ++g) nlike_g[g] += h_nlike_g[(size_t)w * PC_MAX_GRADE + g];
    }

    // ---- waiting for the device.  A run on its own synchronises its stream; a run in step, inside a fiber, yields to the driver,
    //      which launches what all runs have written down, waits once for all of them and resumes them (pc_run_many)
    void sync_point()
    {
        if (fib) {
            fib->yield();
            if (fib->cancel) {      // resumed to unwind, out through the frames of round_finish: what this wait was for stays in the ledger, for destroy()
                fetching.clear(); own_fetches.clear(); staged_up.clear();
                throw FiberCancelled{};
            }
            return;
        }
        if (co) co->flush();
        pc_wait_stream(st);
    }
    // something launched here and now, behind whatever the runs in step have written down so far
    void direct_op() { if (co) co->flush(); }
    // a stage of the round: in step with other runs written down (0), alone launched now by the stage's one-run launch (its return code)
    int stage(const Cohort::Rec &r)
    {
        if (co) { co->rec(r); return 0; }
        return Cohort::stage(r.kind).one(r, st);
    }
    // device -> host, through a pinned block, in stream order behind everything asked for so far; the values are there after fetch_wait()
    struct Fetch { void *h; void *dst; size_t bytes; };
    std::vector<Fetch> fetching;
    void fetch_raw(void *dst, const void *src, size_t bytes)
    {
        if (!bytes) return;
        void *h = blocks.pin<char>(bytes);
        fetching.push_back({h, dst, bytes});
        hipStream_t q = st;
        if (co && batch_copies()) co->post_copies.push_back({(uintptr_t)h, (uintptr_t)src, (uintptr_t)bytes});
        else if (co) co->post.push_back([h, src, bytes, q] { HIPCHK(hipMemcpyAsync(h, src, bytes, hipMemcpyDeviceToHost, q)); });
        // a run on its own: the same rule as in step -- what is asked for comes down at the wait, in ONE kernel (an update with clustering
        // asks for a dozen small arrays: 890 copy commands a run at configs[2], ~7 us of the stream each)
        else if (batch_copies()) own_fetches.push_back({(uintptr_t)h, (uintptr_t)src, (uintptr_t)bytes});
        else HIPCHK(hipMemcpyAsync(h, src, bytes, hipMemcpyDeviceToHost, st));
    }
    template <class T> void fetch(std::vector<T> &v, const T *p, size_t n) { v.resize(n); fetch_raw(v.data(), p, sizeof(T) * n); }
    std::vector<std::array<uintptr_t, 3>> own_fetches;
    void fetch_wait()
    {
        if (!own_fetches.empty()) { std::vector<std::array<uintptr_t, 3>> c; c.swap(own_fetches); pc_copy_many(c, st); }
        sync_point();
        for (Fetch &f : fetching) { std::memcpy(f.dst, f.h, f.bytes); blocks.release(f.h); }
        fetching.clear();
        for (void *&h : staged_up) blocks.release(h);
        staged_up.clear();
    }
    // host -> device, through a pinned block, in stream order (the block goes back at the next wait)
    std::vector<void *> staged_up;
    void send_raw(void *dst, const void *src, size_t bytes)
    {
        if (!bytes) return;
        direct_op();
        void *h = blocks.pin<char>(bytes);
        staged_up.push_back(h);
        std::memcpy(h, src, bytes);
        // (runs in step: with the other copies at the head of the next launch -- what was written down before this call has been launched
        //  by direct_op(), and whatever is launched behind it, here and now or written down, goes through the same door)
        if (co && batch_copies()) co->pre_copies.push_back({(uintptr_t)dst, (uintptr_t)h, (uintptr_t)bytes});
        else HIPCHK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st));
    }

    // host -> device for kernels that are WRITTEN DOWN after this call (runs in step: the copy is made at the start of the common launch,
    // so the runs' kernels stay together; the destination must not be read by anything this run wrote down before)
    void send_pre(void *dst, const void *src, size_t bytes)
    {
        if (!bytes) return;
        if (!co) { send_raw(dst, src, bytes); return; }
        void *h = blocks.pin<char>(bytes);
        staged_up.push_back(h);
        std::memcpy(h, src, bytes);
        hipStream_t q = st;
        if (batch_copies()) co->pre_copies.push_back({(uintptr_t)dst, (uintptr_t)h, (uintptr_t)bytes});
        else co->pre.push_back([dst, h, bytes, q] { HIPCHK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, q)); });
    }
    static bool batch_copies() { return !pc_env().copy_batch_off; }

    void read_ctl()
    {
        fetch_raw(h_ctl_in(), S.ctl, sizeof(PcCtl));
        fetch_wait();
        *h_ctl = ctl_in;
        HIPCHK(hipGetLastError());                    // a kernel that could not be launched must not go unnoticed
        nph_stale = false;
        kt.collect();                                 // (the stream is idle: every open span is complete)
    }
    PcCtl ctl_in;
    PcCtl *h_ctl_in() { return &ctl_in; }

    // The outcome of a round without a copy and without a stream synchronisation: the contraction kernel stamps the
    // host mirror when it is done.  The row copies of the round (k_apply_*) may still be running when this returns;
    // everything the host enqueues next is ordered behind them by the stream.
    void launch_stamp() { S.notify_seq = ++note_seq; }
    unsigned long ready_spins = 0;
    // has the round's contraction kernel reported?  (non-blocking; a stream that finished without a stamp is an error)
    bool round_ready()
    {
        const bool off = pc_env().notify_off;
        if (off || !S.ctl_host) { read_ctl(); return true; }
        const volatile unsigned long long *w = (const volatile unsigned long long *)h_note;
        unsigned long long got[PC_NOTE_WORDS];
        bool all = true;
        for (int i = 0; i < PC_NOTE_WORDS; ++i) { got[i] = w[i]; all = all && (unsigned)(got[i] >> 32) == note_seq; }
        if (!all) {
            if ((++ready_spins & 0x3FFFu) == 0x3FFFu) {
                // nothing after ~a millisecond: did the stream die (launch failure, fault)?  A finished stream without a
                // stamp is an error; a busy one just takes long (general contraction kernel, large nurseries)
                const hipError_t q = hipStreamQuery(st);
                if (q == hipSuccess) {
                    bool ok = true;
                    for (int i = 0; i < PC_NOTE_WORDS; ++i) ok = ok && (unsigned)(w[i] >> 32) == note_seq;
                    if (!ok) engine_fail(PC_RC_DEVICE, "a contraction kernel finished without reporting (launch failure?)");
                } else if (q != hipErrorNotReady) engine_fail(PC_RC_DEVICE, "HIP error %s while waiting for a round", hipGetErrorString(q));
                if (ready_spins > (1ul << 22)) std::this_thread::yield();
            }
            return false;
        }
        PcCtl &c = *h_ctl;
        const int hi_before = c.i_nursery > 0 ? c.i_nursery - 1 : B - 1;       // the segment starts where the last one stopped
        c.status = (int)(got[0] & 0xFF); c.error = (int)((got[0] >> 8) & 0xFF); c.cluster_deleted = (int)((got[0] >> 16) & 1);
        c.upd_pending = (int)((got[0] >> 17) & 1); c.upd_marks = (int)((got[0] >> 18) & 0x3FFF);
        c.i_nursery = (int)((unsigned)got[1] & 0xFFFFu); c.ndead = (int)(unsigned)got[2]; c.nphantom = (int)(unsigned)got[3];
        c.ncluster = (int)(got[4] & 0xFFFF);
        {   // the low 16 bits of a counter that only grows
            int cand = (c.ncluster_dead & ~0xFFFF) | (int)((got[4] >> 16) & 0xFFFF);
            if (cand < c.ncluster_dead) cand += 0x10000;
            c.ncluster_dead = cand;
        }
        c.seg_hi = hi_before; c.seg_lo = c.i_nursery;
        nph_stale = false;
        return true;
    }

    void grow_dead(int nd)
    {
        if (co) co->flush();      // (what the runs in step have written down is launched before an array moves)
        HIPCHK(hipStreamSynchronize(st_copy));        // rows still travelling from the old array
        auto grow = [&](auto *&p, size_t per) { blocks.regrow(p, (size_t)nd * per, (size_t)h_ctl->ndead * per, st); };
        grow(S.dead, S.nT); grow(S.dead_logw, 1); grow(S.dead_postX, 1); grow(S.dead_postZ, 1); grow(S.dead_cuid, 1); grow(S.dead_entry, 1);
        S.Dcap = nd;
        // the pinned mirror the rows are streamed into grows with the array (the same capacities in every run: the block comes
        // back from the cache; sized by the final count at the end it was a fresh multi-GB pinning and a second copy of every row)
        if (h_dead && (size_t)nd > h_dead_cap) { blocks.release(h_dead); h_dead_cap = (size_t)nd; h_dead = blocks.pin<double>(h_dead_cap * S.nT); h_dead_copied = 0; }
    }

    // The reference reallocates its phantom arrays whenever they fill up (run_time_info.f90:747-757 via
    // array_utils reallocate); phantoms are only cleaned at updates, i.e. every -nlive log(compression_factor) deaths,
    // so a small compression_factor needs far more than the initial estimate.
    void grow_phantoms(long long need)
    {
        if (co) co->flush();      // (what the runs in step have written down is launched before an array moves)
        const long long hard = 1LL << 30;             // rows; Pcap and the phantom counters are ints
        if (need > hard) engine_fail(PC_RC_LIMIT, "more than %lld phantom points (%lld needed)", hard, need);
        long long np = std::max<long long>(need, 2LL * S.Pcap);
        np = std::min(np, hard);
        if (g_inject_fault.load() == 3) { g_inject_fault = 0; engine_fail(PC_RC_MEMORY, "out of device memory growing the phantom array to %lld rows (injected)", np); }
        const size_t used = (size_t)std::min<long long>(h_ctl->nphantom, S.Pcap);
        HIPCHK(hipStreamSynchronize(st));
        auto grow = [&](auto *&p, size_t per) { blocks.regrow(p, (size_t)np * per, used * per, st); };
        grow(S.phantom, S.nT); grow(S.ph_logL, 1); grow(S.ph_cuid, 1); grow(S.ph_uid, 1);
        blocks.release(ph2); blocks.release(phL2); blocks.release(phC2); blocks.release(phU2); blocks.release(keep); blocks.release(blk);
        alloc_phantom_side((int)np);
        S.Pcap = (int)np;
    }

    // pool mode: the phantom array is full -- drop what the updates have invalidated (general clean: flags, scan, scatter into
    // the alternate buffers), grow if that is not enough.  Between nurseries only.
    long long pool_cursor = 0;
    // the phantom array is full: the phantoms that are still wanted move to the front of the alternate buffers.  In step with other
    // runs the clean is launched for all of them at once and waited for once (compact_wanted / compact_record / compact_finish)
    bool compact_wanted() const { return S.pool && h_ctl->status == PC_ST_RUNNING && h_ctl->i_nursery == 0 && pool_cursor + (long long)B * S.nr > S.Pcap; }
    void compact_record() { co->rec(rec_compact(S, keep, blk, d_total, ph2, phL2, phC2, phU2, (int)pool_cursor)); }
    void compact_finish(int total)
    {
        std::swap(S.phantom, ph2); std::swap(S.ph_logL, phL2); std::swap(S.ph_cuid, phC2); std::swap(S.ph_uid, phU2);
        pool_cursor = total; h_ctl->nphantom = total; nph_stale = false;
        if (pool_cursor + (long long)B * S.nr > S.Pcap / 2) grow_phantoms(std::max<long long>(2LL * S.Pcap, 2 * (pool_cursor + (long long)B * S.nr)));
        tm.compactions++;
    }
    void pool_compact()
    {
        DbgSpan dbg_t{g_dbg_compact_ns};
        if (co) co->flush();
        hipEvent_t e0 = kt.begin(KT_CLEAN);
        pc_launch_clean(&S, (int)pool_cursor, keep, blk, d_total, ph2, phL2, phC2, phU2, nullptr, st);
        kt.end(KT_CLEAN, e0);
        int total = 0;
        HIPCHK(hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        kt.collect();
        compact_finish(total);
    }
    void ensure_capacity()
    {   // the next batch may append B*nr phantoms and B dead points
        if ((long long)h_ctl->ndead + B + S.Ncap + 16 > S.Dcap) grow_dead(S.Dcap * 2);
        if (S.pool) { if (h_ctl->ncluster_dead + h_ctl->ncluster + 8 > S.maxc_dead) grow_dead_clusters(2 * S.maxc_dead); return; }
        if (nph_stale && (long long)h_ctl->nphantom + (long long)B * S.nr > S.Pcap) read_ctl();   // pre-clean count: refresh
        if ((long long)h_ctl->nphantom + (long long)B * S.nr > S.Pcap) grow_phantoms((long long)h_ctl->nphantom + (long long)B * S.nr);
        // dead clusters: a segment can retire at most the clusters that are active when it starts
        if (h_ctl->ncluster_dead + h_ctl->ncluster + 8 > S.maxc_dead) grow_dead_clusters(2 * S.maxc_dead);
    }

    void grow_dead_clusters(int nd)
    {
        if (co) co->flush();      // (what the runs in step have written down is launched before an array moves)
        HIPCHK(hipStreamSynchronize(st));
        const size_t used = (size_t)std::min(h_ctl->ncluster_dead, S.maxc_dead);
        blocks.regrow(S.logZp_dead, (size_t)nd, used, st); blocks.regrow(S.logZp2_dead, (size_t)nd, used, st); blocks.regrow(S.cl_uid_dead, (size_t)nd, used, st);
        S.maxc_dead = nd;
    }

    // The reference has no limit on the number of clusters (add_cluster reallocates every per-cluster array,
    // run_time_info.f90:392-418).  Here the per-cluster arrays are flat with a capacity: grow them the same way.
    void grow_clusters(int need)
    {
        const int mo = S.maxc, mn = std::max(need, 2 * mo), Ncap = S.Ncap, DD = S.D * S.D;
        if (mn > 16384) engine_fail(PC_RC_LIMIT, "more than 16384 clusters");
        if (co) co->flush();
        HIPCHK(hipStreamSynchronize(st));
        auto grow_d = [&](auto *&p, auto fill) {      // (through the host: the new entries get their initial values)
            using T = std::remove_reference_t<decltype(*p)>;
            std::vector<T> v = dl((const T *)p, (size_t)mo); v.resize(mn, (T)fill);
            blocks.release(p); p = blocks.dev<T>(mn); ul(p, v);
        };
        grow_d(S.logZp, cfg.logzero); grow_d(S.logZXp, cfg.logzero); grow_d(S.logZp2, cfg.logzero); grow_d(S.logZpXp, cfg.logzero);
        grow_d(S.logLp, cfg.logzero); grow_d(S.logXp, 0.0); grow_d(S.lse_ref, 0.0); grow_d(S.lse_sum, 0.0); grow_d(S.death_thr, -PC_HUGE);
        grow_d(S.cl_n, 0); grow_d(S.imin_slot, 0); grow_d(S.cl_uid, 0u);
        {   // the cross-volume matrix changes its leading dimension
            std::vector<double> o = dl(S.XpXq, (size_t)mo * mo), v((size_t)mn * mn, 0.0);
            for (int a = 0; a < mo; ++a) std::copy(o.begin() + (size_t)a * mo, o.begin() + (size_t)(a + 1) * mo, v.begin() + (size_t)a * mn);
            blocks.release(S.XpXq); S.XpXq = blocks.dev<double>(2 * (size_t)mn * mn); ul(S.XpXq, v);
        }
        blocks.regrow(S.cl_list, (size_t)mn * Ncap, (size_t)mo * Ncap, st);
        auto grow_mat = [&](double *&p) {
            double *q = blocks.dev<double>((size_t)mn * DD);
            HIPCHK(hipMemcpy(q, p, sizeof(double) * (size_t)mo * DD, hipMemcpyDeviceToDevice));
            std::vector<double> id((size_t)(mn - mo) * DD, 0.0);
            for (int c = 0; c < mn - mo; ++c) for (int a = 0; a < S.D; ++a) id[(size_t)c * DD + (size_t)a * S.D + a] = 1.0;
            HIPCHK(hipMemcpy(q + (size_t)mo * DD, id.data(), sizeof(double) * id.size(), hipMemcpyHostToDevice));
            blocks.release(p); p = q;
        };
        grow_mat(S.chol); grow_mat(S.cov);
        clus.regrow_counts(mn);
        release_cov(); cov_chunks_cap = 0;   // sized with maxc: covmats() reallocates
        S.maxc = mn;
    }

    // dump (nested_sampling.F90:546-590): live and dead points as [theta, phi, birth, logL] rows,
    // posterior log-weights normalised to logsumexp 0
    // stage 0: update, 1: after the kill-off, 2: the initial live points before any death (prior files)
    void call_dumper(int stage = 0)
    {
        if (!(dumper && stage != 2) && !on_update) return;
        const int nT = S.nT, D = S.D, nDer = S.nDer, npars = D + nDer + 2, nd = h_ctl->ndead;
        HIPCHK(hipStreamSynchronize(st));
        if (nd > hm_ndead) {
            std::vector<double> rows((size_t)(nd - hm_ndead) * nT), lw(nd - hm_ndead);
            hm_cuid.resize(nd);
            HIPCHK(hipMemcpy(hm_cuid.data() + hm_ndead, S.dead_cuid + hm_ndead, sizeof(unsigned) * (nd - hm_ndead), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(rows.data(), S.dead + (size_t)hm_ndead * nT, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(lw.data(), S.dead_logw + hm_ndead, sizeof(double) * lw.size(), hipMemcpyDeviceToHost));
            hm_dead.resize((size_t)nd * npars); hm_logw.resize(nd);
            for (int i = hm_ndead; i < nd; ++i) {
                const double *r = rows.data() + (size_t)(i - hm_ndead) * nT;
                double *o = hm_dead.data() + (size_t)i * npars;
                std::memcpy(o, r + S.p0, sizeof(double) * (D + nDer)); o[D + nDer] = r[S.b0]; o[D + nDer + 1] = r[S.l0];
                hm_logw[i] = lw[i - hm_ndead] + r[S.l0];
            }
            hm_ndead = nd;
        }
        std::vector<double> lwn(hm_logw.begin(), hm_logw.begin() + nd);
        double m = -PC_HUGE;
        for (double v : lwn) m = std::max(m, v);
        double sum = 0.0;
        for (double v : lwn) sum += std::exp(v - m);
        const double lse = m + std::log(sum);
        for (double &v : lwn) v -= lse;
        // live points ordered by cluster, then list position
        auto lc = dl(S.live_cluster, S.Ncap); auto lp = dl(S.live_pos, S.Ncap); auto lr = dl(S.live, (size_t)S.Ncap * nT);
        std::vector<std::pair<long long, int>> ord;
        for (int s = 0; s < S.Ncap; ++s) if (lc[s] >= 0) ord.push_back({(long long)lc[s] * S.Ncap + lp[s], s});
        std::sort(ord.begin(), ord.end());
        std::vector<double> live(std::max<size_t>(1, ord.size()) * npars);
        for (size_t k = 0; k < ord.size(); ++k) {
            const double *r = lr.data() + (size_t)ord[k].second * nT;
            double *o = live.data() + k * npars;
            std::memcpy(o, r + S.p0, sizeof(double) * (D + nDer)); o[D + nDer] = r[S.b0]; o[D + nDer + 1] = r[S.l0];
        }
        const double lz = std::max(-PC_HUGE, 2 * h_ctl->logZ - 0.5 * h_ctl->logZ2), var = h_ctl->logZ2 - 2 * h_ctl->logZ;
        double dummy = 0.0;
        if (dumper && stage != 2) dumper(nd, (int)ord.size(), npars, live.data(), nd > 0 ? hm_dead.data() : &dummy, nd > 0 ? lwn.data() : &dummy, lz, std::sqrt(std::fabs(var)));
        if (on_update) {
            const int nc = h_ctl->ncluster, ncd = std::min(h_ctl->ncluster_dead, S.maxc_dead);
            std::vector<int> lcl(std::max<size_t>(1, ord.size()));
            for (size_t k = 0; k < ord.size(); ++k) lcl[k] = lc[ord[k].second];
            auto zp = dl(S.logZp, std::max(1, nc)), zp2 = dl(S.logZp2, std::max(1, nc));
            auto zd = dl(S.logZp_dead, std::max(1, ncd)), zd2 = dl(S.logZp2_dead, std::max(1, ncd));
            auto cn = dl(S.cl_n, std::max(1, nc));
            std::vector<double> e1(std::max(1, nc)), s1(std::max(1, nc)), e2(std::max(1, ncd)), s2(std::max(1, ncd));
            for (int i = 0; i < nc; ++i) { e1[i] = 2 * zp[i] - 0.5 * zp2[i]; s1[i] = std::sqrt(std::fabs(zp2[i] - 2 * zp[i])); }   // run_time_info.f90:652-678
            for (int i = 0; i < ncd; ++i) { e2[i] = 2 * zd[i] - 0.5 * zd2[i]; s2[i] = std::sqrt(std::fabs(zd2[i] - 2 * zd[i])); }
            pchip_update u{};
            u.final_call = stage; u.ndiscarded = ndiscarded; u.ndead = nd; u.nlive = (int)ord.size(); u.npars = npars;
            u.dead = nd > 0 ? hm_dead.data() : &dummy; u.logpost = nd > 0 ? hm_logw.data() : &dummy;
            u.live = live.data(); u.live_cluster = lcl.data();
            u.logZ = lz; u.logZerr = std::sqrt(std::fabs(var)); u.nlike = h_ctl->nlike;
            long ng[PC_MAX_GRADE]; int gdims[PC_MAX_GRADE];
            grade_counts(ng);
            for (int g = 0; g < S.ngrade; ++g) gdims[g] = (g + 1 < S.ngrade ? S.g_off[g + 1] : D) - S.g_off[g];
            u.ngrade = S.ngrade; u.nlike_grade = ng; u.grade_dims = gdims; u.grade_repeats = S.g_nr;
            u.ncluster = nc; u.ncluster_dead = ncd; u.nlive_p = cn.data();
            u.logZp = e1.data(); u.logZperr = s1.data(); u.logZp_dead = e2.data(); u.logZperr_dead = s2.data();
            auto ua = dl(S.cl_uid, std::max(1, nc)); auto ud = dl(S.cl_uid_dead, std::max(1, ncd));
            unsigned dummy_u = 0u;
            u.dead_cluster = nd > 0 ? hm_cuid.data() : &dummy_u; u.cluster_uid = ua.data(); u.cluster_uid_dead = ud.data();
            u.nsplit = (int)split_child.size(); u.split_child = split_child.data(); u.split_parent = split_parent.data();
            u.split_logfrac = split_logfrac.data();
            u.n_extra = (int)pp_logpost.size(); u.extra = pp_rows.data(); u.extra_logpost = pp_logpost.data(); u.extra_cluster = pp_cuid.data(); u.extra_uid = pp_uid.data();
            on_update(hook_user, &u);
        }
    }

    // clean_phantoms + calculate_covmats (nested_sampling.F90:326-368 minus file output / clustering)
    // clean_phantoms also feeds the posterior (run_time_info.f90:845-870): a phantom that falls below the contour is
    // kept with probability thin_posterior = boost_posterior / num_repeats (generate.F90:311-316) and carries the
    // weight of the first point of its cluster that died since the last update with a larger logL.  Host side: the
    // feature is off by default and touches each phantom once per update.
    void collect_phantom_posteriors(int nph)
    {
        const double thin = cfg.boost_posterior < 0.0 ? 1.0 : cfg.boost_posterior / (double)S.nr;
        const int nd0 = nd_last_update, nd = h_ctl->ndead, nT = S.nT, np = S.D + S.nDer;
        nd_last_update = nd;
        if (!(thin > 0.0) || nph <= 0 || nd <= nd0) return;
        HIPCHK(hipStreamSynchronize(st));
        auto kp = dl(keep, nph); auto phL = dl(S.ph_logL, nph); auto phC = dl(S.ph_cuid, nph); auto phU = dl(S.ph_uid, nph);
        const int m = nd - nd0;
        std::vector<double> dL(m), dW = dl(S.dead_logw + nd0, m); auto dC = dl(S.dead_cuid + nd0, m);
        HIPCHK(hipMemcpy2D(dL.data(), sizeof(double), S.dead + (size_t)nd0 * nT + S.l0, sizeof(double) * nT, sizeof(double), m, hipMemcpyDeviceToHost));
        std::map<unsigned, std::vector<std::pair<double, double>>> stack;      // per cluster: (logL, logweight), death order
        for (int i = 0; i < m; ++i) if (dW[i] > cfg.logzero) stack[dC[i]].push_back({dL[i], dW[i]});
        std::vector<int> pick; std::vector<double> pickw;
        for (int j = 0; j < nph; ++j) {
            if (kp[j]) continue;
            const unsigned long long uid = phU[j];
            if (!(polychord_hip_keyed_uniform((unsigned)cfg.seed, PC_DOM_PHANTOM, (unsigned)(uid >> 32), (unsigned)uid, 0u) < thin)) continue;
            auto it = stack.find(phC[j]);
            if (it == stack.end()) continue;
            const auto &v = it->second;
            // deaths of one cluster arrive in ascending logL: first entry above the phantom
            size_t lo = 0, hi = v.size();
            while (lo < hi) { const size_t mid = (lo + hi) / 2; if (v[mid].first > phL[j]) hi = mid; else lo = mid + 1; }
            if (lo == v.size()) continue;
            pick.push_back(j); pickw.push_back(v[lo].second);
        }
        if (pick.empty()) return;
        std::vector<double> row(nT);
        for (size_t k = 0; k < pick.size(); ++k) {
            HIPCHK(hipMemcpy(row.data(), S.phantom + (size_t)pick[k] * nT, sizeof(double) * nT, hipMemcpyDeviceToHost));
            const size_t o = pp_rows.size();
            pp_rows.resize(o + np + 2);
            std::memcpy(pp_rows.data() + o, row.data() + S.p0, sizeof(double) * np);
            pp_rows[o + np] = row[S.b0]; pp_rows[o + np + 1] = row[S.l0];
            pp_logpost.push_back(pickw[k] + row[S.l0]); pp_cuid.push_back(phC[pick[k]]); pp_uid.push_back(phU[pick[k]]);
        }
    }

    // Sequential-stream test mode with posteriors = T: clean_phantoms draws one Bernoulli uniform for every phantom it
    // removes (run_time_info.f90:857-859, even when thin_posterior = 0), all from the one generator: the engine's stream
    // position moves on by as many, so that the next nursery draws what the reference binary's draws.  (The trials of
    // update_posteriors for equals = T depend on the order of the reference's arrays and are not emulated: with
    // equals = T the sequential mode is a valid run, not the reference's.)
    void seq_consume(unsigned long long n)
    {
        if (!n) return;
        h_ctl->seq += n;
        HIPCHK(hipMemcpy(&S.ctl->seq, &h_ctl->seq, sizeof(unsigned long long), hipMemcpyHostToDevice));
    }

    // what a sampling launch of this run alone is counted under besides its kernel (live points, nurseries)
    PcLaunchTraits launch_traits() const { return PcLaunchTraits{pc_rtc_wanted(&S) != 0, src_terms, S.prior.kind >= PCHIP_PRIOR_TABLE}; }
    PcUpdateFacts update_facts(int nph) const { return PcUpdateFacts{nph > 0, pc_update_fused_ok(&S, h_ctl->ncluster) != 0, h_ctl->ncluster}; }

    void do_update(bool deferred = false)
    {
        tm.updates += deferred ? std::max(1, h_ctl->upd_marks) : 1;
        // the round loop only sees the compact notification; whoever looks at evidences, counters or cluster ids gets the block
        const bool seq_post = S.seq_mode && (cfg.posteriors || cfg.equals);
        if (plan.ctl == PC_CTL_EARLY) { const int st_keep = h_ctl->status; read_ctl(); h_ctl->status = st_keep; }
        if (!plan.hook_late) call_dumper();
        const int nph = S.pool ? (int)pool_cursor : h_ctl->nphantom;
        const PcUpdateChoice upd = pc_choose_update(plan, update_facts(nph));
        pc_count(path, upd);
        if (upd.kind == PC_UPDATE_FUSED) {
            const size_t need = (size_t)pc_update_fused_blocks(&S, nph) * pc_update_fused_entries(&S);
            if (need > upd_part_cap) { blocks.release(upd_part); upd_part_cap = 2 * need; upd_part = blocks.dev<double>(upd_part_cap); }
            if (!upd_shift) {
                upd_shift = blocks.dev<double>(S.D);
                std::vector<double> half(S.D, 0.5);               // first update: moments about the centre of the hypercube
                HIPCHK(hipMemcpyAsync(upd_shift, half.data(), sizeof(double) * S.D, hipMemcpyHostToDevice, st));
                HIPCHK(hipStreamSynchronize(st));
            }
            hipEvent_t e0 = kt.begin(KT_CLEAN);
            // (the flags of these rows came with the round's row kernel: round_enqueue)
            if (!co && deferred && r_flagged && r_flag_nph == nph && r_flag_keep == keep && r_flag_blk == blk)
                pc_launch_update_fused_at(&S, nph, keep, blk, d_total, ph2, phL2, phC2, phU2, upd_part, upd_shift, 1, 1, st);
            else
            (void)stage(rec_update(S, keep, blk, d_total, ph2, phL2, phC2, phU2, upd_part, upd_shift, co ? pc_update_fused_grid(&S, nph, deferred ? 1 : 0) : 0, deferred, nph));
            r_flagged = false;
            kt.end(KT_CLEAN, e0);
            if (upd.need_count) {
                // (in step with other runs the update was only written down: the copy of its count comes behind its launch)
                std::vector<int> tot;
                fetch(tot, (const int *)d_total, 1);
                fetch_wait();
                const int total = tot[0];
                h_ctl->nphantom = total;
                if (seq_post) seq_consume((unsigned long long)(nph - total));
            } else nph_stale = true;
            if (!S.pool) { std::swap(S.phantom, ph2); std::swap(S.ph_logL, phL2); std::swap(S.ph_cuid, phC2); std::swap(S.ph_uid, phU2); }
            write_resume();
            return;
        }
        if (deferred) engine_fail(PC_RC_DEVICE, "deferred update without the fused update path");
        hipEvent_t e0 = kt.begin(KT_CLEAN);
        // (in step with other runs: the clean of all runs that update in this round is one launch, like the pool compaction)
        // (... of no rows: nothing to write down, launched now behind what has been)
        if (co && nph <= 0) { direct_op(); pc_launch_clean(&S, nph, keep, blk, d_total, ph2, phL2, phC2, phU2, nullptr, st); }
        else (void)stage(rec_compact(S, keep, blk, d_total, ph2, phL2, phC2, phU2, nph));
        kt.end(KT_CLEAN, e0);
        if (plan.hook_late) { collect_phantom_posteriors(nph); call_dumper(); }
        // The surviving count is written to the control block on the device.  Without clustering / resume files
        // nothing on the host needs it before the next round's read-back, so the update costs no extra sync: the
        // covariance grid is sized with the pre-clean count and the kernels clamp to the device value.
        const bool need_count = upd.need_count, ctl_late = upd.ctl == PC_CTL_LATE;
        int total = nph;
        std::vector<int> tot, cn;
        if (need_count) {
            fetch(tot, (const int *)d_total, 1);
            if (cfg.do_clustering) fetch(cn, (const int *)S.cl_n, (size_t)h_ctl->ncluster);      // (the clusters' sizes for do_clustering: the same wait)
            if (ctl_late) fetch_raw(&ctl_in, S.ctl, sizeof(PcCtl));
        } else nph_stale = true;
        std::swap(S.phantom, ph2); std::swap(S.ph_logL, phL2); std::swap(S.ph_cuid, phC2); std::swap(S.ph_uid, phU2);
        (void)stage(rec_reset(S));
        if (need_count) {
            fetch_wait();
            if (ctl_late) { const int st_keep = h_ctl->status; *h_ctl = ctl_in; h_ctl->status = st_keep; nph_stale = false; }
            total = tot[0];
            h_ctl->nphantom = total;
            if (seq_post) seq_consume((unsigned long long)(nph - total));
        }
        if (cfg.do_clustering) {
            // nested_sampling.F90:352-367: the sub-dimension pass first, then the full one over every cluster there is after it (the sizes
            // fetched again when the first pass split); the chains in the nursery follow the list through both (cmap_total)
            if (sub_dims.empty()) clus.do_clustering(cn);
            else {
                const int nold = h_ctl->ncluster;
                std::vector<int> map1, map2;
                path[PCHIP_PATH_SUBCLUSTER_PASSES]++;
                const long s0 = nsplits;
                bool found = clus.do_clustering(cn, c_subdims, (int)sub_dims.size(), &map1);
                if (found) { path[PCHIP_PATH_SUBCLUSTER_SPLITS] += nsplits - s0; cn.clear(); }      // (the full pass asks for the sizes again)
                found = clus.do_clustering(cn, nullptr, 0, &map2) || found;
                cluster_map_compose(map1, map2);                              // the update's cluster j -> its place after both passes
                if (found && !cfg.epoch_discard) clus.remap_nursery(map1, nold);
            }
        }
        hipEvent_t e1 = kt.begin(KT_COV);
        covmats(total, h_ctl->ncluster);
        kt.end(KT_COV, e1);
        write_resume();                               // nested_sampling.F90:337
    }

    // (in stream order, through pinned blocks: a run in step shares the wait with the others)
    template <class T> std::vector<T> dl(const T *p, size_t n)
    {
        std::vector<T> v;
        fetch(v, p, n);
        fetch_wait();
        return v;
    }
    template <class T> void ul(T *p, const std::vector<T> &v) { send_raw(p, v.data(), sizeof(T) * v.size()); }

    void release_cov() { blocks.release(psum); blocks.release(pcnt); blocks.release(pcov); blocks.release(mean); blocks.release(count); }
    void covmats(int nph, int nc)
    {
        const size_t nchunk = pc_cov_nchunk(&S, nph);
        if (nchunk * nc > cov_chunks_cap) {
            release_cov();
            cov_chunks_cap = nchunk * nc * 2;
            psum = blocks.dev<double>(cov_chunks_cap * S.D); pcnt = blocks.dev<int>(cov_chunks_cap);
            pcov = blocks.dev<double>(cov_chunks_cap * S.D * S.D);
            mean = blocks.dev<double>((size_t)S.maxc * S.D); count = blocks.dev<int>(S.maxc);
        }
        direct_op();
        if (pc_launch_covmats(&S, nph, nc, psum, pcnt, mean, count, pcov, st)) {
            engine_fail(PC_RC_LDS, "covariance tile exceeds LDS (nDims too large)");
        }
    }

    // prior + likelihood on the host for one hypercube point (calculate.f90:40-41)
    double host_eval(const double *cube, double *theta, double *phi)
    {
        const int D = S.D;
        if (cb_prior) cb_prior(const_cast<double *>(cube), theta, D);
        else if (have_ptab) pc_prior_table_eval(ptab, cube, theta);
        else {
            if ((int)h_lo.size() != D) {
                h_lo.assign(D, 0.0); h_hi.assign(D, 1.0);
                if (d_lo) { HIPCHK(hipMemcpy(h_lo.data(), d_lo, sizeof(double) * D, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(h_hi.data(), d_hi, sizeof(double) * D, hipMemcpyDeviceToHost)); }
            }
            for (int d = 0; d < D; ++d) theta[d] = h_lo[d] + (h_hi[d] - h_lo[d]) * cube[d];
        }
        cb_evals++;
        return cb_like(theta, D, phi, S.nDer);
    }

    // prior + likelihood for n hypercube points at once: one call of the registered batch callback, else n scalar calls
    void host_eval_batch(int n, const double *cubes, double *thetas, double *phis, double *logLs)
    {
        const int D = S.D, nDer = S.nDer, pd = std::max(1, nDer);
        if (batch_fn) { batch_fn(batch_user, n, D, nDer, cubes, thetas, phis, logLs); cb_evals += n; return; }
        for (int i = 0; i < n; ++i) logLs[i] = host_eval(cubes + (size_t)i * D, thetas + (size_t)i * D, phis + (size_t)i * pd);
    }

    void generate_live_callback()
    {   // GenerateLivePoints with host evaluations; same Philox streams as k_generate_live
        const int nprior = cfg.nprior <= 0 ? cfg.nlive : cfg.nprior, nT = S.nT, D = S.D;
        std::vector<double> rows((size_t)nprior * nT, 0.0);
        int have = 0; uint32_t attempt = 0; long long nlike = 0;
        double t_eval = 0.0;
        const int pd = std::max(1, S.nDer);
        std::vector<double> bc, bt, bp, bl;
        while (have < nprior) {
            // as many attempts as points are still missing (all of them valid is the common case); attempt numbers,
            // and with them the Philox streams, are those of one-at-a-time generation
            const int m = nprior - have;
            bc.resize((size_t)m * D); bt.resize((size_t)m * D); bp.assign((size_t)m * pd, 0.0); bl.resize(m);
            for (int i = 0; i < m; ++i)
                for (int d = 0; d < D; ++d) bc[(size_t)i * D + d] = h_uniform(S.k0, S.k1, PC_DOM_LIVEGEN, 0u, attempt + (uint32_t)i, (uint32_t)d);
            const auto te0 = std::chrono::steady_clock::now();
            host_eval_batch(m, bc.data(), bt.data(), bp.data(), bl.data());
            t_eval += std::chrono::duration<double>(std::chrono::steady_clock::now() - te0).count();
            if (stop.load(std::memory_order_relaxed)) return;
            for (int i = 0; i < m; ++i) {
                if (!(bl[i] > cfg.logzero)) continue;
                double *row = rows.data() + (size_t)have * nT;
                std::copy(bc.begin() + (size_t)i * D, bc.begin() + (size_t)(i + 1) * D, row);
                std::copy(bt.begin() + (size_t)i * D, bt.begin() + (size_t)(i + 1) * D, row + S.p0);
                std::copy(bp.begin() + (size_t)i * pd, bp.begin() + (size_t)i * pd + S.nDer, row + S.d0);
                row[S.b0] = cfg.logzero; row[S.l0] = bl[i];
                have++; nlike++;
            }
            attempt += (uint32_t)m;
            if (attempt > 1000u * (uint32_t)nprior + 100000u) engine_fail(PC_RC_SETTINGS, "could not generate live points (likelihood is logzero everywhere?)");
        }
        double *drows = blocks.dev<double>((size_t)nprior * nT);
        HIPCHK(hipMemcpy(drows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
        pc_launch_install_live(&S, drows, nprior, st);
        h_ctl->nlike = nlike;
        HIPCHK(hipMemcpyAsync(&S.ctl->nlike, &h_ctl->nlike, sizeof(long long), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        blocks.release(drows);
        ndiscarded = (long)attempt - nprior;
        cb_eval_seconds = attempt ? t_eval / attempt : -1.0;
        call_dumper(2);
        if (nprior > cfg.nlive) { pc_count(path, PcTrimLive{}); pc_launch_consume(&S, 2, 0, st); read_ctl(); }
    }

    // one nursery batch in callback mode: tick the chains until all of them are done
    void slice_callback(unsigned batch)
    {
        const int D = S.D, nDer = S.nDer;
        int first = 1;
        while (true) {
            // answers of the host: [logL (B) | theta (B x D) | phi (B x nDerived)], device copy at d_ans (B = chains per nursery now)
            pc_launch_slice_tick(&S, batch, B, d_cs, d_x0s, d_decks, d_prop, d_ans, d_ans + B, d_ans + B + (size_t)B * D, first, hp_prop, hp_need, st);
            first = 0; cb_ticks++;
            HIPCHK(hipStreamSynchronize(st));
            if (stop.load(std::memory_order_relaxed)) return;
            double *evL = hp_ans, *evT = hp_ans + B, *evP = evT + (size_t)B * D;
            const int pd = std::max(1, nDer);
            int nneed = 0;
            if (batch_fn) {                                // the parked proposals of this round in one call
                cb_idx.clear();
                for (int c = 0; c < B; ++c) if (hp_need[c]) cb_idx.push_back(c);
                nneed = (int)cb_idx.size();
                if (nneed > 0) {
                    cb_c.resize((size_t)nneed * D); cb_t.resize((size_t)nneed * D); cb_p.assign((size_t)nneed * pd, 0.0); cb_l.resize(nneed);
                    for (int i = 0; i < nneed; ++i) std::copy(hp_prop + (size_t)cb_idx[i] * D, hp_prop + (size_t)(cb_idx[i] + 1) * D, cb_c.begin() + (size_t)i * D);
                    host_eval_batch(nneed, cb_c.data(), cb_t.data(), cb_p.data(), cb_l.data());
                    for (int i = 0; i < nneed; ++i) {
                        const int c = cb_idx[i];
                        evL[c] = cb_l[i];
                        std::copy(cb_t.begin() + (size_t)i * D, cb_t.begin() + (size_t)(i + 1) * D, evT + (size_t)c * D);
                        std::copy(cb_p.begin() + (size_t)i * pd, cb_p.begin() + (size_t)(i + 1) * pd, evP + (size_t)c * pd);
                    }
                    if (stop.load(std::memory_order_relaxed)) return;
                }
            } else
            for (int c = 0; c < B; ++c)
                if (hp_need[c]) { nneed++; evL[c] = host_eval(hp_prop + (size_t)c * D, evT + (size_t)c * D, evP + (size_t)c * pd); }
            if (nneed == 0) break;
            HIPCHK(hipMemcpyAsync(d_ans, hp_ans, sizeof(double) * (size_t)B * (1 + D + std::max(1, nDer)), hipMemcpyHostToDevice, st));
        }
    }

    // ---- the device batch callback (polychord_hip_set_device_batch_callback): the blocks stay on the device ----
    // prior (box or table: the engine's, on the block) + the caller's function for the n cubes in db_cube; everything is enqueued on the
    // run's stream, nothing is waited for here
    void device_eval_batch(int n)
    {
        tick_answered(n);
        device_call(n);
    }
    // ... the two halves of it.  In step the group makes ONE call for the rows of all its runs, through the first of them that ticked
    // (device_call with the group's total), and every run that had rows in it counts the call and its own rows (tick_answered)
    void device_call(int n)
    {
        if (db_flags && pc_launch_prior_transform(&S_pri, n, db_cube, db_theta, st)) engine_fail(PC_RC_NDIMS, "the device prior of the batch callback could not be launched (nDims = %d)", S.D);
        if (dbatch_fn(dbatch_user, n, S.D, S.nDer, db_cube, db_theta, db_phi, db_logL, db_flags, (void *)st) != 0) stop.store(1);
    }
    void tick_answered(int n)
    {
        path[PCHIP_PATH_DEVICE_BATCH]++; cb_evals += n;
        if (qb_nres > 0) path[PCHIP_PATH_SOURCE_KERNELS] += 2 * (long)((n + qb_rows - 1) / qb_rows);      // (k_quad_residuals and k_quad_finish of every slab)
    }
    // the group's block in place of the run's own four (which served the live points, and go back now: the stream is idle behind begin())
    void tick_bind(double *cube, double *theta, double *phi, double *logL)
    {
        blocks.release(db_cube); blocks.release(db_theta); blocks.release(db_phi); blocks.release(db_logL);
        db_cube = cube; db_theta = theta; db_phi = phi; db_logL = logL; tick_shared = true;
    }

    void generate_live_device()
    {   // generate_live_callback without the host: the same attempts and Philox coordinates, drawn by k_live_cubes; only the logL values come
        // down, to choose the valid rows, which k_live_gather puts together for k_install_live
        const int nprior = cfg.nprior <= 0 ? cfg.nlive : cfg.nprior, nT = S.nT;
        double *drows = blocks.dev<double>((size_t)nprior * nT), *h_l = blocks.pin<double>(nprior);
        int *d_idx = blocks.dev<int>(nprior), *h_idx = blocks.pin<int>(nprior);
        int have = 0; uint32_t attempt = 0; long long nlike = 0;
        double t_eval = 0.0;
        while (have < nprior) {
            const int m = nprior - have;
            pc_launch_live_cubes(&S, attempt, m, db_cube, st);
            const auto te0 = std::chrono::steady_clock::now();
            device_eval_batch(m);
            if (stop.load(std::memory_order_relaxed)) return;      // (the blocks go back with the ledger)
            HIPCHK(hipMemcpyAsync(h_l, db_logL, sizeof(double) * m, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            t_eval += std::chrono::duration<double>(std::chrono::steady_clock::now() - te0).count();
            if (stop.load(std::memory_order_relaxed)) return;
            int nv = 0;
            for (int i = 0; i < m; ++i) if (h_l[i] > cfg.logzero) h_idx[nv++] = i;
            if (nv > 0) {
                HIPCHK(hipMemcpyAsync(d_idx, h_idx, sizeof(int) * nv, hipMemcpyHostToDevice, st));
                pc_launch_live_gather(&S, nv, d_idx, db_cube, db_theta, db_phi, db_logL, drows + (size_t)have * nT, st);
                HIPCHK(hipStreamSynchronize(st));                   // (h_idx and the blocks are written again by the next attempt)
            }
            have += nv; nlike += nv;
            attempt += (uint32_t)m;
            if (attempt > 1000u * (uint32_t)nprior + 100000u) engine_fail(PC_RC_SETTINGS, "could not generate live points (likelihood is logzero everywhere?)");
        }
        pc_launch_install_live(&S, drows, nprior, st);
        h_ctl->nlike = nlike;
        HIPCHK(hipMemcpyAsync(&S.ctl->nlike, &h_ctl->nlike, sizeof(long long), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        blocks.release(drows); blocks.release(h_l); blocks.release(d_idx); blocks.release(h_idx);
        ndiscarded = (long)attempt - nprior;
        cb_eval_seconds = attempt ? t_eval / attempt : -1.0;
        call_dumper(2);
        if (nprior > cfg.nlive) { pc_count(path, PcTrimLive{}); pc_launch_consume(&S, 2, 0, st); read_ctl(); }
    }

    // one nursery batch through the device callback.  A round: the tick (answers at the ranks of the last pack), the pack (index kernel,
    // row kernel), ONE wait for the count, the prior on the block if it is the engine's, the caller's function
    void slice_device(unsigned batch)
    {
        int first = 1, stride = 1, off = 0;
        pc_chain_need_layout(&stride, &off);
        if (co) {
            // In step: the tick is written down, the group is told where the flags, the proposals and the ranks are, and the run yields.  The
            // driver launches the ticks of all runs that wait once, packs their proposals into the one block, waits once and calls the
            // caller's function once (pc_step.h, enqueue_as_fibers); the run's own count says whether it is done.
            if (!fib || !tick_shared) engine_fail(PC_RC_DEVICE, "a device batch callback in step outside its group's tick phase");
            while (true) {
                co->rec(rec_tick(S, batch, B, d_cs, d_x0s, d_decks, d_prop, db_logL, db_theta, db_phi, db_rank, first != 0));
                first = 0; cb_ticks++;
                tick_want = PcParkRun{(const int *)d_cs + off, d_prop, db_rank, B, stride}; tick_asked = true;
                fib->yield();
                if (fib->cancel) throw FiberCancelled{};      // (resumed to unwind: another run failed)
                if (stop.load(std::memory_order_relaxed)) return;
                if (tick_count == 0) break;
            }
            return;
        }
        while (true) {
            pc_launch_slice_tick_dev(&S, batch, B, d_cs, d_x0s, d_decks, d_prop, db_logL, db_theta, db_phi, first, db_rank, st);
            first = 0; cb_ticks++;
            pc_launch_park_pack(B, S.D, (const int *)d_cs + off, stride, d_prop, db_rank, db_count, hp_count_dev, db_cube, st);
            HIPCHK(hipStreamSynchronize(st));
            if (stop.load(std::memory_order_relaxed)) return;
            const int n = *(volatile int *)hp_count;
            if (n == 0) break;
            device_eval_batch(n);
            if (stop.load(std::memory_order_relaxed)) return;
        }
    }

    void generate_live()
    {   // GenerateLivePoints (generate.F90:150-183): keep the first nprior valid prior samples
        const int nprior = cfg.nprior <= 0 ? cfg.nlive : cfg.nprior, nT = S.nT;
        double *rows = blocks.dev<double>((size_t)nprior * nT), *rl = blocks.dev<double>(nprior);
        std::vector<double> keep_rows; keep_rows.reserve((size_t)nprior * nT);
        std::vector<double> hrows, hl(nprior);        // (hrows: only when a prior sample was not valid -- 736 KB zeroed for nothing was a third of a run's set-up)
        int have = 0, attempt0 = 0, last_attempt = -1;
        long long nlike = 0;
        bool direct = true;
        while (have < nprior) {
            pc_count(path, launch_traits());
            if (pc_launch_generate_live(&S, attempt0, nprior, rows, rl, st)) {
                if (pc_rtc_wanted(&S) && pc_rtc_error()) engine_fail(PC_RC_SETTINGS, "%.480s", pc_rtc_error());
                engine_fail(PC_RC_NDIMS, "nDims > 256 unsupported");
            }
            HIPCHK(hipMemcpyAsync(hl.data(), rl, sizeof(double) * nprior, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            int nvalid = 0;
            for (int i = 0; i < nprior; ++i) nvalid += hl[i] > cfg.logzero;
            if (nvalid == nprior && have == 0) { have = nprior; nlike = nprior; last_attempt = nprior - 1; break; }   // common case: all valid
            direct = false;
            hrows.resize((size_t)nprior * nT);
            HIPCHK(hipMemcpy(hrows.data(), rows, sizeof(double) * (size_t)nprior * nT, hipMemcpyDeviceToHost));
            for (int i = 0; i < nprior && have < nprior; ++i)
                if (hl[i] > cfg.logzero) { keep_rows.insert(keep_rows.end(), hrows.begin() + (size_t)i * nT, hrows.begin() + (size_t)(i + 1) * nT); have++; nlike++; last_attempt = attempt0 + i; }
                else ndiscarded++;
            attempt0 += nprior;
        }
        if (!direct) HIPCHK(hipMemcpy(rows, keep_rows.data(), sizeof(double) * (size_t)nprior * nT, hipMemcpyHostToDevice));
        pc_launch_install_live(&S, rows, nprior, st);
        h_ctl->nlike = nlike; h_ctl->nlike_device = nlike;
        HIPCHK(hipMemcpyAsync(&S.ctl->nlike, &h_ctl->nlike, sizeof(long long), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        if (S.seq_mode) {
            // the reference draws and evaluates one more prior sample while it times the likelihood
            // (time_speeds, generate.F90:388-393); the stream position after it is where the sampling starts.
            // With explicit repeats for every grade it does not (generate.F90:285-287).
            int a = last_attempt + 1;
            for (; S.ngrade <= 1; ++a) {
                double l1 = 0.0;
                pc_count(path, launch_traits());
                (void)pc_launch_generate_live(&S, a, 1, rows, rl, st);
                HIPCHK(hipMemcpyAsync(&l1, rl, sizeof(double), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                if (l1 > cfg.logzero) break;
            }
            h_ctl->seq = (unsigned long long)(a + (S.ngrade <= 1 ? 1 : 0)) * S.D;
            HIPCHK(hipMemcpy(&S.ctl->seq, &h_ctl->seq, sizeof(unsigned long long), hipMemcpyHostToDevice));
        }
        blocks.release(rows); blocks.release(rl);
        call_dumper(2);                // write_prior_file, nested_sampling.F90:197
        if (nprior > cfg.nlive) {      // nested_sampling.F90:201-205
            pc_count(path, PcTrimLive{}); pc_launch_consume(&S, 2, 0, st);
            read_ctl();
        }
    }

    // Dead rows are append-only: everything below ctl.ndead is final once the round's kernels have been
    // synchronised, so it can travel to the pinned result buffer on a second stream during the run.
    void stream_dead()
    {
        const size_t nd = (size_t)h_ctl->ndead;
        if (!h_dead || nd > h_dead_cap || nd <= h_dead_copied) return;
        if (ev_apply) HIPCHK(hipStreamWaitEvent(st_copy, ev_apply, 0));     // the rows are written by k_apply_dead_ph, which may still run
        HIPCHK(hipMemcpyAsync(h_dead + h_dead_copied * S.nT, S.dead + h_dead_copied * S.nT,
                              sizeof(double) * (nd - h_dead_copied) * S.nT, hipMemcpyDeviceToHost, st_copy));
        h_dead_copied = nd;
    }

    // ---- .resume (pc_resume.h): the sampler state at an update boundary, in the reference's own grammar
    void export_resume(PcResume &r)
    {
        HIPCHK(hipStreamSynchronize(st));
        const int D = S.D, nT = S.nT, nc = h_ctl->ncluster, ncd = std::min(h_ctl->ncluster_dead, S.maxc_dead), maxc = S.maxc;
        r = PcResume{};
        r.nDims = D; r.nDerived = S.nDer; r.ndead = h_ctl->ndead; r.ncluster = nc; r.ncluster_dead = ncd;
        {
            long ng[PC_MAX_GRADE];
            grade_counts(ng);
            r.grade_dims.clear(); r.num_repeats.clear(); r.nlike.clear();
            for (int g = 0; g < S.ngrade; ++g) {
                r.grade_dims.push_back((g + 1 < S.ngrade ? S.g_off[g + 1] : D) - S.g_off[g]);
                r.num_repeats.push_back(S.g_nr[g]); r.nlike.push_back(ng[g]);
            }
        }
        r.logZ = h_ctl->logZ; r.logZ2 = h_ctl->logZ2; r.logX_last_update = h_ctl->logX_last_update;
        r.thin_posterior = cfg.boost_posterior < 0.0 ? 1.0 : cfg.boost_posterior / (double)S.nr;      // generate.F90:311-316
        auto take = [&](const double *p) { auto v = dl(p, std::max(1, nc)); v.resize(nc); return v; };
        r.logLp = take(S.logLp); r.logXp = take(S.logXp); r.logZXp = take(S.logZXp); r.logZp = take(S.logZp);
        r.logZp2 = take(S.logZp2); r.logZpXp = take(S.logZpXp);
        auto xq = dl(S.XpXq, (size_t)maxc * maxc);
        r.logXpXq.assign((size_t)nc * nc, 0.0);
        for (int q = 0; q < nc; ++q) for (int p = 0; p < nc; ++p) r.logXpXq[(size_t)q * nc + p] = xq[(size_t)p * maxc + q];
        r.logZp_dead = dl(S.logZp_dead, std::max(1, ncd)); r.logZp_dead.resize(ncd);
        r.logZp2_dead = dl(S.logZp2_dead, std::max(1, ncd)); r.logZp2_dead.resize(ncd);
        auto cov = dl(S.cov, (size_t)std::max(1, nc) * D * D), ch = dl(S.chol, (size_t)std::max(1, nc) * D * D);
        r.covmat.assign((size_t)nc * D * D, 0.0); r.cholesky.assign((size_t)nc * D * D, 0.0);
        for (int c = 0; c < nc; ++c) for (int j = 0; j < D; ++j) for (int a = 0; a < D; ++a) {     // file line j = column j
            r.covmat[((size_t)c * D + j) * D + a] = cov[((size_t)c * D + a) * D + j];
            r.cholesky[((size_t)c * D + j) * D + a] = ch[((size_t)c * D + a) * D + j];
        }
        auto cn = dl(S.cl_n, std::max(1, nc)); auto cl = dl(S.cl_list, (size_t)maxc * S.Ncap);
        auto rows = dl(S.live, (size_t)S.Ncap * nT); auto uid = dl(S.cl_uid, std::max(1, nc));
        r.nlive.assign(nc, 0); r.imin.assign(nc, 1); r.live.assign(nc, {}); r.nphantom.assign(nc, 0); r.phantom.assign(nc, {});
        for (int c = 0; c < nc; ++c) {
            r.nlive[c] = cn[c];
            double lo = PC_HUGE;
            for (int k = 0; k < cn[c]; ++k) {
                const double *row = rows.data() + (size_t)cl[(size_t)c * S.Ncap + k] * nT;
                r.live[c].insert(r.live[c].end(), row, row + nT);
                if (row[S.l0] < lo) { lo = row[S.l0]; r.imin[c] = k + 1; }
            }
        }
        const int nph = h_ctl->nphantom;
        auto ph = dl(S.phantom, (size_t)std::max(1, nph) * nT); auto pc = dl(S.ph_cuid, std::max(1, nph));
        for (int j = 0; j < nph; ++j)
            for (int c = 0; c < nc; ++c)
                if (uid[c] == pc[j]) { r.phantom[c].insert(r.phantom[c].end(), ph.begin() + (size_t)j * nT, ph.begin() + (size_t)(j + 1) * nT); r.nphantom[c]++; break; }
        r.dead = dl(S.dead, (size_t)std::max(1, r.ndead) * nT); r.dead.resize((size_t)r.ndead * nT);
        r.logweights = dl(S.dead_logw, std::max(1, r.ndead)); r.logweights.resize(r.ndead);
    }

    // The reference's .resume grammar has no place for what this engine derives its posterior files from: the cluster
    // every dead point died in (a stable id), the genealogy of the splits with the evidence fractions, the phantoms kept
    // by boost_posterior.  They travel in a sidecar next to the file, <path>.hip (binary, this engine only); a run that
    // resumes from a .resume without it -- one the reference wrote -- has the evidences and the global posterior of
    // the dead points, and per-cluster posteriors from the resume point on.
    void write_sidecar(const std::string &path, int ndead, int nc, int ncd)
    {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) engine_fail(PC_RC_RESUME, "cannot write %s", path.c_str());
        auto put = [&](const void *p, size_t n) { if (n && std::fwrite(p, 1, n, f) != n) { std::fclose(f); engine_fail(PC_RC_RESUME, "short write to %s", path.c_str()); } };
        const unsigned magic = 0x50434831u;   // "PCH1"
        const int np = S.D + S.nDer + 2, nsplit = (int)split_child.size(), npp = (int)pp_logpost.size();
        const unsigned next_uid = h_ctl->next_cluster_uid;
        auto dc = dl(S.dead_cuid, (size_t)std::max(1, ndead)); auto ua = dl(S.cl_uid, (size_t)std::max(1, nc)); auto ud = dl(S.cl_uid_dead, (size_t)std::max(1, ncd));
        put(&magic, 4); put(&ndead, 4); put(&nc, 4); put(&ncd, 4); put(&next_uid, 4); put(&nsplit, 4); put(&npp, 4); put(&np, 4);
        put(dc.data(), sizeof(unsigned) * ndead); put(ua.data(), sizeof(unsigned) * nc); put(ud.data(), sizeof(unsigned) * ncd);
        put(split_child.data(), sizeof(unsigned) * nsplit); put(split_parent.data(), sizeof(unsigned) * nsplit); put(split_logfrac.data(), sizeof(double) * nsplit);
        put(pp_rows.data(), sizeof(double) * (size_t)npp * np); put(pp_logpost.data(), sizeof(double) * npp); put(pp_cuid.data(), sizeof(unsigned) * npp);
        std::fclose(f);
    }
    struct Sidecar { bool ok = false; unsigned next_uid = 1; std::vector<unsigned> dead_cuid, uid, uid_dead; };
    Sidecar read_sidecar(const std::string &path, int ndead, int nc, int ncd)
    {
        Sidecar sc;
        FILE *f = std::fopen(path.c_str(), "rb");
        if (!f) return sc;
        auto get = [&](void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; };
        unsigned magic = 0; int nd = 0, c = 0, cd = 0, nsplit = 0, npp = 0, np = 0;
        bool good = get(&magic, 4) && magic == 0x50434831u && get(&nd, 4) && get(&c, 4) && get(&cd, 4) && get(&sc.next_uid, 4) &&
                    get(&nsplit, 4) && get(&npp, 4) && get(&np, 4) && nd == ndead && c == nc && cd == ncd && np == S.D + S.nDer + 2 &&
                    nsplit >= 0 && npp >= 0;
        if (good) {
            sc.dead_cuid.resize(nd); sc.uid.resize(c); sc.uid_dead.resize(cd);
            split_child.resize(nsplit); split_parent.resize(nsplit); split_logfrac.resize(nsplit);
            pp_rows.resize((size_t)npp * np); pp_logpost.resize(npp); pp_cuid.resize(npp);
            good = get(sc.dead_cuid.data(), sizeof(unsigned) * nd) && get(sc.uid.data(), sizeof(unsigned) * c) && get(sc.uid_dead.data(), sizeof(unsigned) * cd) &&
                   get(split_child.data(), sizeof(unsigned) * nsplit) && get(split_parent.data(), sizeof(unsigned) * nsplit) &&
                   get(split_logfrac.data(), sizeof(double) * nsplit) && get(pp_rows.data(), sizeof(double) * (size_t)npp * np) &&
                   get(pp_logpost.data(), sizeof(double) * npp) && get(pp_cuid.data(), sizeof(unsigned) * npp);
        }
        std::fclose(f);
        if (!good) { split_child.clear(); split_parent.clear(); split_logfrac.clear(); pp_rows.clear(); pp_logpost.clear(); pp_cuid.clear(); }
        // (the kept phantoms' ids do not travel in the sidecar: after a resume the earlier ones are numbered -- ids only key the equal-weight trials)
        pp_uid.resize(pp_logpost.size()); for (size_t k = 0; k < pp_uid.size(); ++k) pp_uid[k] = (1ull << 62) | k;
        sc.ok = good;
        return sc;
    }

    void write_resume()
    {
        if (!cfg.resume_write) return;
        PcResume r;
        export_resume(r);
        std::string err;
        if (!pc_resume_write(cfg.resume_write, r, cfg.logzero, err)) engine_fail(PC_RC_RESUME, "%s", err.c_str());
        write_sidecar(std::string(cfg.resume_write) + ".hip", r.ndead, r.ncluster, r.ncluster_dead);
    }

    // upload a .resume state; the run continues with the counter RNG streams of batch `ndead` onwards
    // (the reference does not store its generator state either: a resumed run is a valid, different trajectory)
    bool import_resume(const PcResume &r, std::string &err)
    {
        const int D = S.D, nT = S.nT, nc = r.ncluster, Ncap = S.Ncap;
        if (r.nDims != D || r.nDerived != S.nDer) { err = "resume file has different nDims / nDerived"; return false; }
        if (nc > S.maxc) grow_clusters(nc);
        if (r.ncluster_dead + nc + 8 > S.maxc_dead) grow_dead_clusters(2 * (r.ncluster_dead + nc + 8));
        const int maxc = S.maxc;
        int ntot = 0, nph = 0;
        for (int c = 0; c < nc; ++c) { ntot += r.nlive[c]; nph += r.nphantom[c]; }
        // ncluster = 0: the file of a finished run (every live point killed): nothing left to sample, the run
        // returns what the file holds, as the reference does
        if (ntot > Ncap || (nc >= 1 && ntot < 1)) { err = "resume file: live point counts do not fit this run's settings"; return false; }
        if (nph + (long long)B * S.nr > S.Pcap) { h_ctl->nphantom = 0; grow_phantoms(nph + (long long)B * S.nr); }
        if ((long long)r.ndead + B + Ncap + 16 > S.Dcap) { h_ctl->ndead = 0; grow_dead(2 * (r.ndead + B + Ncap + 16)); }
        std::vector<double> rows((size_t)Ncap * nT, 0.0), lL(Ncap, PC_HUGE), entry(Ncap, cfg.logzero);
        std::vector<int> lc(Ncap, -1), lp(Ncap, 0), cl((size_t)maxc * Ncap, 0), cn(maxc, 0), imin(maxc, 0);
        std::vector<unsigned> uid(maxc, 0u);
        const Sidecar sc = cfg.resume_read ? read_sidecar(std::string(cfg.resume_read) + ".hip", r.ndead, nc, std::min(r.ncluster_dead, S.maxc_dead)) : Sidecar{};
        std::vector<double> logLp(maxc, cfg.logzero), lref(maxc, 0.0), lsum(maxc, 0.0);
        int slot = 0;
        for (int c = 0; c < nc; ++c) {
            cn[c] = r.nlive[c]; uid[c] = sc.ok ? sc.uid[c] : (unsigned)(c + 1);
            double lo = PC_HUGE, hi = -PC_HUGE;
            for (int k = 0; k < r.nlive[c]; ++k, ++slot) {
                const double *row = r.live[c].data() + (size_t)k * nT;
                std::memcpy(rows.data() + (size_t)slot * nT, row, sizeof(double) * nT);
                lL[slot] = row[S.l0]; lc[slot] = c; lp[slot] = k; entry[slot] = row[S.b0]; cl[(size_t)c * Ncap + k] = slot;
                if (row[S.l0] < lo) { lo = row[S.l0]; imin[c] = slot; }
                hi = std::max(hi, row[S.l0]);
            }
            logLp[c] = r.nlive[c] ? lo : cfg.logzero;
            lref[c] = r.nlive[c] ? hi : 0.0;
            for (int k = 0; k < r.nlive[c]; ++k) lsum[c] += std::exp(r.live[c][(size_t)k * nT + S.l0] - lref[c]);
        }
        ul(S.live, rows); ul(S.live_logL, lL); ul(S.live_entry, entry); ul(S.live_cluster, lc); ul(S.live_pos, lp);
        { std::vector<int> none(Ncap, -1); ul(S.slot_src, none); }     // every live row is current (k_install_live does this in a fresh run)
        ul(S.cl_list, cl); ul(S.cl_n, cn); ul(S.cl_uid, uid); ul(S.imin_slot, imin); ul(S.logLp, logLp); ul(S.lse_ref, lref); ul(S.lse_sum, lsum);
        auto put = [&](double *dst, const std::vector<double> &v) { std::vector<double> t(maxc, cfg.logzero); std::copy(v.begin(), v.end(), t.begin()); ul(dst, t); };
        put(S.logZp, r.logZp); put(S.logZXp, r.logZXp); put(S.logZp2, r.logZp2); put(S.logZpXp, r.logZpXp);
        { std::vector<double> t(maxc, 0.0); std::copy(r.logXp.begin(), r.logXp.end(), t.begin()); ul(S.logXp, t); }
        std::vector<double> xq((size_t)maxc * maxc, 0.0);
        for (int q = 0; q < nc; ++q) for (int p = 0; p < nc; ++p) xq[(size_t)p * maxc + q] = r.logXpXq[(size_t)q * nc + p];
        ul(S.XpXq, xq);
        std::vector<double> cov((size_t)maxc * D * D, 0.0), ch((size_t)maxc * D * D, 0.0);
        for (int c = 0; c < maxc; ++c) for (int a = 0; a < D; ++a) { cov[((size_t)c * D + a) * D + a] = 1.0; ch[((size_t)c * D + a) * D + a] = 1.0; }
        for (int c = 0; c < nc; ++c) for (int j = 0; j < D; ++j) for (int a = 0; a < D; ++a) {
            cov[((size_t)c * D + a) * D + j] = r.covmat[((size_t)c * D + j) * D + a];
            ch[((size_t)c * D + a) * D + j] = r.cholesky[((size_t)c * D + j) * D + a];
        }
        ul(S.cov, cov); ul(S.chol, ch);
        const int ncd = std::min(r.ncluster_dead, S.maxc_dead);
        { std::vector<double> a(r.logZp_dead.begin(), r.logZp_dead.begin() + ncd), b(r.logZp2_dead.begin(), r.logZp2_dead.begin() + ncd); ul(S.logZp_dead, a); ul(S.logZp2_dead, b); }
        if (sc.ok) ul(S.cl_uid_dead, sc.uid_dead);
        // phantoms, cluster by cluster
        std::vector<double> ph((size_t)std::max(1, nph) * nT), phL(std::max(1, nph));
        std::vector<unsigned> phC(std::max(1, nph)); std::vector<unsigned long long> phU(std::max(1, nph));
        int j = 0;
        for (int c = 0; c < nc; ++c)
            for (int k = 0; k < r.nphantom[c]; ++k, ++j) {
                std::memcpy(ph.data() + (size_t)j * nT, r.phantom[c].data() + (size_t)k * nT, sizeof(double) * nT);
                phL[j] = ph[(size_t)j * nT + S.l0]; phC[j] = uid[c]; phU[j] = 0xFFFFFFFF00000000ull | (unsigned)j;
            }
        if (nph) { ul(S.phantom, ph); ul(S.ph_logL, phL); ul(S.ph_cuid, phC); ul(S.ph_uid, phU); }
        // dead points
        if (r.ndead) {
            ul(S.dead, r.dead); ul(S.dead_logw, r.logweights);
            std::vector<double> z(r.ndead, 0.0), en(r.ndead);
            for (int i = 0; i < r.ndead; ++i) en[i] = r.dead[(size_t)i * nT + S.b0];
            ul(S.dead_postX, z); ul(S.dead_postZ, z); ul(S.dead_entry, en);
            std::vector<unsigned> du(r.ndead, 0u);
            if (sc.ok) du = sc.dead_cuid;
            ul(S.dead_cuid, du);
        }
        PcCtl c0 = *h_ctl;
        c0.status = nc >= 1 ? PC_ST_RUNNING : PC_ST_DONE; c0.ncluster = nc; c0.ncluster_dead = ncd; c0.ndead = r.ndead; c0.nphantom = nph;
        c0.logZ = r.logZ; c0.logZ2 = r.logZ2; c0.logX_last_update = r.logX_last_update; c0.next_cluster_uid = sc.ok ? sc.next_uid : (unsigned)nc + 1;
        c0.nlike = 0;                                  // the engine's counter is the total over the grades
        for (size_t g = 0; g < r.nlike.size(); ++g) { c0.nlike += r.nlike[g]; if (g >= 1 && g < PC_MAX_GRADE) nlike_g[g] = r.nlike[g]; }
        c0.nlike_device = c0.nlike; c0.i_nursery = 0; c0.failures = 0;
        HIPCHK(hipMemcpy(S.ctl, &c0, sizeof(PcCtl), hipMemcpyHostToDevice));
        *h_ctl = c0;
        return true;
    }

    // ---- a run in phases, so that ONE host thread can keep several runs of a device in flight (pchip_run_repeats): begin(),
    //      then round_enqueue() / round_ready() / round_finish() until it says stop, then end().  run() is the same sequence
    //      for a single run, spinning in between.  State that lives across the phases:
    struct ActiveRun {
        int d; std::atomic<int> *flag;
        ActiveRun(int dv, std::atomic<int> *f) : d(dv & 63), flag(f) { g_active_runs.fetch_add(1); g_active_dev[d].fetch_add(1); std::lock_guard<std::mutex> g(g_run_mutex); g_run_stop.push_back(flag); }
        ~ActiveRun() { g_active_runs.fetch_sub(1); g_active_dev[d].fetch_sub(1); std::lock_guard<std::mutex> g(g_run_mutex); g_run_stop.erase(std::find(g_run_stop.begin(), g_run_stop.end(), flag)); }
    };
    std::unique_ptr<ActiveRun> active_run;
    using clk = std::chrono::steady_clock;
    clk::time_point r_t0, r_t1, r_t2;
    unsigned r_batch = 0; bool r_sort_valid = false, r_fresh = false; int r_nursery_left = 0;
    PcRunPlan plan{};                             // which kernels this run may take: made once, at the end of begin() (pc_plan.h)
    int r_rc = 0;                                 // outcome of the loop: 0, or the code run() returns

    int run(pchip_result *out)
    {
        int rc = begin();
        if (rc >= 0) return rc;
        while (true) {
            if (!round_enqueue()) break;
            while (!round_ready()) __builtin_ia32_pause();
            if (!round_finish()) break;
        }
        if (r_rc != 0) return r_rc;
        return end(out);
    }

    // everything before the first round; -1: go on, else the code to return
    int begin()
    {
        active_run.reset(new ActiveRun(dev, &stop));
        r_t0 = clk::now();
        h_dead_cap = (size_t)S.Dcap; h_dead = blocks.pin<double>(h_dead_cap * S.nT); h_dead_copied = 0;
        bool resumed = false;
        if (cfg.resume_read) {                         // read_write.F90:384-476; a missing file means a fresh start
            if (FILE *probe = std::fopen(cfg.resume_read, "r")) {
                std::fclose(probe);
                PcResume rs; std::string err;
                if (!pc_resume_read(cfg.resume_read, rs, err) || !import_resume(rs, err)) { std::fprintf(stderr, "polychord_hip: %s\n", err.c_str()); return 6; }
                resumed = true;
                int ntot = 0;
                for (int v : rs.nlive) ntot += v;
                if (ntot > cfg.nlive && rs.ncluster == 1) { pc_count(path, PcTrimLive{}); pc_launch_consume(&S, 2, 0, st); read_ctl(); ntot = cfg.nlive; }   // nested_sampling.F90:201-205
                resume_static = (ntot == cfg.nlive);
                resume_batch0 = (unsigned)rs.ndead;
            }
        }
        if (!resumed) { if (dev_batch) generate_live_device(); else if (callback_mode) generate_live_callback(); else generate_live(); }
        if (stop.load(std::memory_order_relaxed)) return 5;
        if (cb_auto_batch && !(cb_eval_seconds >= 0.0 && cb_eval_seconds < 2e-6)) { B = B_small; S.B = B; }   // expensive (or unmeasured) callback
        r_t1 = clk::now();
        r_batch = resume_batch0;                      // fresh counter-RNG streams after a resume
        r_sort_valid = false;
        r_nursery_left = 0;
        make_plan();
        S.defer_update = plan.defer ? 1 : 0; S.pool = plan.pool ? 1 : 0;
        r_flagged = false;
        if (S.pool) {
            pool_cursor = h_ctl->nphantom;
            if (g_cap_phantoms.load() <= 0) {                                    // room for several updates between compactions,
                size_t free_b = 0, total_b = 0;                                  // where the device has it to spare
                (void)hipMemGetInfo(&free_b, &total_b);
                const double need = 2.0 * 2.0 * (double)S.Pcap * ((double)S.nT * 8.0 + 24.0);       // both buffers at twice the rows
                if (need < 0.4 * (double)free_b) grow_phantoms(2LL * S.Pcap);
            }
        }
        r_rc = 0;
        return -1;
    }

    // the run's plan: the launchers' predicates whose inputs are fixed from here on are asked here
    void make_plan()
    {
        const int nprior0 = cfg.nprior <= 0 ? cfg.nlive : cfg.nprior;
        PcRunFacts f{};
        f.ablate = cfg.ablate; f.force_general = cfg.force_general;
        f.fixed_nlive = (cfg.n_nlives == 0) && (nprior0 >= cfg.nlive) && resume_static;
        f.par_fits = pc_par_fits(&S) != 0; f.fast_fits = pc_fast_fits(&S) != 0; f.fused_fits_one = pc_update_fused_ok(&S, 1) != 0;
        f.clustering = cfg.do_clustering != 0; f.boost = cfg.boost_posterior != 0.0;
        f.dumper = dumper != nullptr; f.on_update = on_update != nullptr; f.resume_write = cfg.resume_write != nullptr;
        f.seq_mode = S.seq_mode != 0; f.posteriors = cfg.posteriors || cfg.equals;
        f.callback = callback_mode;
        plan = pc_plan_run(f);
    }
    // another run is at work on this device, in step with this one or not
    bool other_active() const { return g_active_dev[dev & 63].load(std::memory_order_relaxed) > 1; }
    // what the cohort's launches for any device likelihood take (else the run launches for itself in between)
    bool cohort_general_ok() const
    {
        // (a device prior and a source likelihood included: pc_launch_slice_step, pc_cohort.h)
        return !pc_env().cohort_general_off && S.ngrade <= 1 && !S.seq_mode && S.like.kind != PC_LIKE_CORR_GAUSSIAN && S.like.kind != PC_LIKE_CALLBACK;
    }
    // what is known when a nursery is about to be sampled (the launchers' predicates: asked here, once a nursery)
    PcNurseryFacts nursery_facts(unsigned batch) const
    {
        PcNurseryFacts f{};
        f.in_step = co != nullptr; f.other_active = other_active(); f.callback = callback_mode; f.D = S.D;
        f.ring = raw_buf[1] != nullptr;
        const RawSlot &rs = ring[batch % raw_depth];
        f.slot_ready = rs.valid && rs.batch == batch && rs.B == B;
        f.second_stream = co && co->st2 && raw_depth >= 2;
        f.splittable = pc_nhats_splittable(&S) != 0; f.fusable = pc_slice_fusable(&S) != 0; f.bases_t = pc_bases_t_ok(&S) != 0;
        f.slice_t = pc_slice_t_ok(&S, h_ctl->ncluster) != 0;
        f.cohort_general = cohort_general_ok();
        f.traits = launch_traits();
        return f;
    }
    // The sampling of one nursery: pool rows, the bases (drawn ahead on the side stream, or now), k_slice, the bases of the
    // nurseries to come.  Which of them: pc_choose_nursery.
    bool enqueue_nursery()
    {
        unsigned &batch = r_batch; int &nursery_left = r_nursery_left;
        if (S.pool) {
            if (pool_cursor + (long long)B * S.nr > S.Pcap) pool_compact();
            S.pool_base = (int)pool_cursor; S.pool_rows = B * S.nr; S.babies = S.phantom + (size_t)pool_cursor * S.nT;
            pool_cursor += (long long)B * S.nr;
        }
        {
            // (between the stamp of the last round and the launch of k_slice the device idles: nothing that can wait
            //  is done in between -- capacity checks precede the contraction, not the sampling)
            hipEvent_t e0 = kt.begin(KT_NHATS);
            const PcNurseryChoice ch = pc_choose_nursery(plan, nursery_facts(batch));
            pc_count(path, ch);
            pc_count_step(path, ch);
            int bases_seq = 0;                        // in step with other runs: the number of the launch that drew this nursery's bases (0: in line)
            switch (ch.bases) {
            case PC_BASES_READY: case PC_BASES_PART1: case PC_BASES_PART1_STEP: {
                RawSlot &rs = ring[batch % raw_depth];
                S.nhat_raw = raw_buf[batch % raw_depth];
                if (ch.bases == PC_BASES_READY) { if (!rs.waited) HIPCHK(hipStreamWaitEvent(st, rs.ready, 0)); bases_seq = rs.co_seq; }      // (in step with other runs: the wait for the launch that drew them, Cohort::flush)
                else {
                    if (rs.valid) HIPCHK(hipStreamWaitEvent(st, rs.ready, 0));       // (a stale job may still be writing there)
                    // (not stage(): a run on its own passes its packed flag, the row's one-run launch 1)
                    if (ch.bases == PC_BASES_PART1_STEP) co->rec(rec_bases(S, batch, B));
                    else (void)pc_launch_nhats_part(&S, batch, B, 1, st, pc_part1_kind(ch.packed, cfg.ablate));
                }
                rs.valid = false;
                if (ch.part2) { if (co) { co->flush(); co->wait_next(); } (void)pc_launch_nhats_part(&S, batch, B, 2, st, 0); }
                break;
            }
            // (not stage(): CK_NHATS_G exists in step only, a run on its own reports a failing launch)
            case PC_BASES_NHATS_G: co->rec(rec_nhats_g(S, batch, B)); break;
            case PC_BASES_WHOLE:
                if (co) co->flush();
                if (pc_launch_nhats(&S, batch, B, st)) { std::fprintf(stderr, "polychord_hip: nDims unsupported\n"); r_rc = 3; return false; }
                break;
            }
            kt.end(KT_NHATS, e0);
            hipEvent_t e1 = kt.begin(KT_SLICE);
            switch (ch.sampler) {
            case PC_SAMPLER_CALLBACK:
                if (co) co->flush();
                if (dev_batch) slice_device(batch); else slice_callback(batch);
                if (stop.load(std::memory_order_relaxed)) { r_rc = 5; return false; }
                break;
            case PC_SAMPLER_LANE: { Cohort::Rec r = rec_slice(S, batch, B, bases_seq); r.note = co ? &step_note : nullptr; (void)stage(r); break; }
            // (not stage(): no run on its own comes here -- its launch is the case below, which counts other paths and reports a failure)
            case PC_SAMPLER_WAVE_STEP: co->rec(rec_slice_g(S, batch, B, ch.fused, ch.fused ? bases_seq : 0, &step_note)); break;
            case PC_SAMPLER_WAVE:
                if (co) { co->flush(); co->wait_next(); }
                if (ch.fused ? pc_launch_slice_fused(&S, batch, B, st) : pc_launch_slice(&S, batch, B, st)) {
                    if (pc_rtc_wanted(&S) && pc_rtc_error()) { std::fprintf(stderr, "polychord_hip: %s\n", pc_rtc_error()); r_rc = 1; return false; }
                    std::fprintf(stderr, "polychord_hip: nDims unsupported\n"); r_rc = 3; return false;
                }
                break;
            }
            if (ch.ahead == PC_AHEAD_STEP) bases_ahead(batch);
            kt.end(KT_SLICE, e1);
            if (ch.ahead == PC_AHEAD_SIDE) side_prefetch(batch);
            if (S.ngrade > 1) HIPCHK(hipMemcpyAsync(h_nlike_g.data(), S.ch_nlike_g, sizeof(int) * h_nlike_g.size(), hipMemcpyDeviceToHost, st));
            batch++; tm.batches++;
            S.nn_valid = 0; nursery_left = B;
        }
        return true;
    }

    // in step with other runs: the bases of the nursery after `cur`, if they are not drawn yet, written down for the cohort's second
    // stream (one ahead: two ahead were slower in step, CHANGELOG.md)
    void bases_ahead(unsigned cur)
    {
        const unsigned x = cur + 1;
        RawSlot &rn = ring[x % raw_depth];
        if (rn.valid && rn.batch == x && rn.B == B) return;
        PcState S1 = S; S1.nhat_raw = raw_buf[x % raw_depth];
        co->rec(rec_bases_next(S1, x, B));      // (in step only)
        rn.valid = true; rn.batch = x; rn.B = B; rn.waited = true; rn.co_seq = co->seq_for_next();
    }

    void ensure_side()
    {
        if (st_side) return;
        st_side = stream_beside({st, st_copy}); ev_main = hpool().get_sync_event();
        for (int r = 0; r < raw_depth; ++r) { ring[r].ready = hpool().get_sync_event(); ring[r].consumed = hpool().get_sync_event(); }
    }
    // Several clusters, a run on its own: the sorted order of the live set (k_sort_live: one workgroup, 17-26 us + a launch) is what the
    // candidate lists and the one-wave contraction start from, and it depends on the live set only -- which the sampling of a fresh
    // nursery does not touch.  It is made on the side stream while k_slice runs; the main stream waits for it in front of the lists.
    hipEvent_t ev_presort_a = nullptr, ev_presort_b = nullptr;
    bool presorted = false;
    void presort_live()
    {
        presorted = false;
        if (pc_env().presort_off || co || other_active() || callback_mode || S.seq_mode || !S.nn_list || h_ctl->ncluster < 2) return;
        ensure_side();
        if (!ev_presort_a) { ev_presort_a = hpool().get_sync_event(); ev_presort_b = hpool().get_sync_event(); }
        HIPCHK(hipEventRecord(ev_presort_a, st)); HIPCHK(hipStreamWaitEvent(st_side, ev_presort_a, 0));      // (behind the row copies of the round before)
        if (pc_launch_sort_live(&S, st_side) != 0) return;
        HIPCHK(hipEventRecord(ev_presort_b, st_side));
        presorted = true;
    }
    // the bases of the nurseries after `cur`, on the side stream (behind cur's sampling kernel on the main stream)
    void side_prefetch(unsigned cur)
    {
        const unsigned batch = cur;
        {
                // drawn while the one-CU contraction of this nursery runs: next to k_slice (one wave per SIMD) the
        // 2000 workgroups of the bases kernel cost it 10 us, next to the contraction nothing
        ensure_side();
        // (nDims > 64: the bases take longer than the contraction and the slice kernel is one wave per SIMD for
        //  half a millisecond: there they run next to it from the start)
        const bool side_free = pc_env().side_free || (S.D > 64 && !pc_env().side_ordered);
        // the buffer of this nursery is free again once its bases have been whitened (fused: once sampled)
        // (ordered: the side stream follows k_slice anyway -- one event between k_slice and the contraction, not two:
        //  every record on the main stream is a few microseconds before the next kernel starts)
        RawSlot &cur = ring[batch % raw_depth];
        if (side_free) { HIPCHK(hipEventRecord(cur.consumed, st)); cur.used = true; }
        if (!side_free) { HIPCHK(hipEventRecord(ev_main, st)); HIPCHK(hipStreamWaitEvent(st_side, ev_main, 0)); }
        // ordered: the next nursery only; free: as far ahead as there are buffers (the last one is this nursery's own)
        const unsigned xmax = batch + (unsigned)raw_depth - (side_free ? 0u : 1u);
        for (unsigned x = batch + 1; x <= xmax; ++x) {
            RawSlot &rs = ring[x % raw_depth];
            if (rs.valid && rs.batch == x && rs.B == B) continue;
            if (rs.valid) continue;                                          // (a job for another nursery size: used or replaced when its turn comes)
            if (rs.used) HIPCHK(hipStreamWaitEvent(st_side, rs.consumed, 0));
            PcState S1 = S; S1.nhat_raw = raw_buf[x % raw_depth];
            hipEvent_t es = kt.begin_on(KT_SIDE, st_side);
            (void)pc_launch_nhats_part(&S1, x, B, 1, st_side, pc_part1_kind((cfg.ablate & PC_ABL_BASES_PACKED) != 0, cfg.ablate));
            kt.end_on(KT_SIDE, es, st_side);
            HIPCHK(hipEventRecord(rs.ready, st_side));
            rs.valid = true; rs.batch = x; rs.B = B; rs.waited = false;
        }
    }
    }

    // what is known when a round's contraction is about to be launched
    PcContractFacts contract_facts(int nursery_left) const
    {
        PcContractFacts f{};
        f.ncluster = h_ctl->ncluster; f.nursery_left = nursery_left;
        f.in_step = co != nullptr; f.cohort_general = cohort_general_ok();
        f.nn_lists = S.nn_list && !pc_env().nn_lists_off; f.nn_valid = S.nn_valid != 0;
        f.cl_fits = f.ncluster > 1 && pc_consume_cl_fits(&S, f.ncluster) != 0;
        f.clp_fits = f.cl_fits && pc_consume_clp_fits(&S, f.ncluster) != 0;
        return f;
    }
    // enqueue one round (sampling when the nursery is empty, contraction, row copies); false: the loop is over (r_rc says how)
    bool round_enqueue()
    {
        unsigned &batch = r_batch; bool &sort_valid = r_sort_valid; int &nursery_left = r_nursery_left;
        {
            if (h_ctl->status == PC_ST_DONE) return false;
            if (h_ctl->status == PC_ST_ERROR) { std::fprintf(stderr, "polychord_hip: device error %d\n", h_ctl->error); r_rc = 2; return false; }
            if (step_note.failed) {      // (in step: the sampling launch of the round before was taken neither for the group nor for this run alone)
                if (pc_rtc_wanted(&S) && pc_rtc_error()) { std::fprintf(stderr, "polychord_hip: %s\n", pc_rtc_error()); r_rc = 1; return false; }
                std::fprintf(stderr, "polychord_hip: nDims unsupported\n"); r_rc = 3; return false;
            }
            bool fresh_nursery = false;
            if (h_ctl->i_nursery == 0) {
                fresh_nursery = true;
                DbgSpan dbg_t{g_dbg_nursery_ns};
                if (plan.cl_ok) presort_live();
                if (!enqueue_nursery()) return false;
            }
            if (fresh_nursery) { DbgSpan dbg_t{g_dbg_capacity_ns}; ensure_capacity(); }
            hipEvent_t e2 = kt.begin(KT_CONSUME);
            int rc2 = 0;
            const PcContractChoice ch = pc_choose_contract(plan, contract_facts(nursery_left));
            pc_count(path, ch);
            launch_stamp();
            if (presorted && (co || !(h_ctl->ncluster > 1))) { HIPCHK(hipStreamWaitEvent(st, ev_presort_b, 0)); presorted = false; }
            switch (ch.kind) {
            case PC_CONTRACT_PAR:
                S.nn_valid = 0;                              // (the one-cluster kernels do not keep the list bookkeeping)
                if (!sort_valid) { rc2 = stage(rec_sort(S)); sort_valid = true; }
                rc2 = rc2 || stage(rec_consume(S));      // also lays out the phantoms
                break;
            case PC_CONTRACT_FAST:
                if (co) co->flush();
                sort_valid = false; S.nn_valid = 0;
                rc2 = pc_launch_consume_fast(&S, 0, st); pc_launch_ph_prepare(&S, st);
                break;
            case PC_CONTRACT_CL_STEP:
                // (not stage(), the three of them: a run on its own passes the lists whether the sort was made now and the contraction the
                //  number of clusters, the rows' one-run launches 1 and 65 or 2)
                sort_valid = false;
                if (ch.want_nn) { co->rec(rec_nn(S, nursery_left)); S.nn_valid = 1; }
                co->rec(rec_sort(S));
                co->rec(rec_consume_cl(S, h_ctl->ncluster > 64));
                break;
            case PC_CONTRACT_CL: case PC_CONTRACT_GENERAL: {
                sort_valid = false;
                if (co) co->flush();
                bool sorted_now = false;
                if (presorted) { HIPCHK(hipStreamWaitEvent(st, ev_presort_b, 0)); sorted_now = fresh_nursery; presorted = false; }      // (made beside k_slice: presort_live)
                if (ch.want_nn) {
                    // (the sorted order first: its ranks tell the lists' kernel which candidates cannot die before a chain is looked at)
                    if (!sorted_now) sorted_now = pc_launch_sort_live(&S, st) == 0;
                    pc_launch_nn_lists(&S, nursery_left, sorted_now ? 1 : 0, st);
                    S.nn_valid = 1;
                }
                if (ch.kind == PC_CONTRACT_CL) rc2 = (sorted_now ? 0 : pc_launch_sort_live(&S, st)) || pc_launch_consume_cl(&S, h_ctl->ncluster, st);
                else rc2 = pc_launch_consume(&S, 0, (h_ctl->ncluster > 1) ? 1 : 0, st);
                break;
            }
            }
            if (rc2) { std::fprintf(stderr, "polychord_hip: nlive too large for the LDS-resident contraction\n"); r_rc = 4; return false; }
            kt.end(KT_CONSUME, e2);
            hipEvent_t e3 = kt.begin(KT_APPLY);
            // a run on its own in pool mode whose updates are deferred and fused: the flag pass of an update that this contraction may leave pending
            // rides in the row kernel's launch (the device knows by then, the host does not yet); do_update starts behind it
            r_flagged = !co && S.pool && S.defer_update && plan.fused_update && ch.kind == PC_CONTRACT_PAR && pool_cursor >= 1 && keep && blk &&
                        !(S.ablate & (PC_ABL_FLAG_LAUNCH | PC_ABL_UPDATE_CHAIN));
            if (r_flagged) {
                r_flag_nph = (int)pool_cursor; r_flag_keep = keep; r_flag_blk = blk;
                pc_launch_apply_flag(&S, batch - 1, B, r_flag_nph, keep, blk, st);
            } else
            (void)stage(rec_apply(S, batch - 1, B));
            kt.end(KT_APPLY, e3);
            // the main stream's wait for the next nursery's bases is enqueued now, behind this round's kernels (long
            // satisfied when the next k_slice gets there), not between the stamp and the next launch
            if (st_side) { RawSlot &rs = ring[batch % raw_depth]; if (rs.valid && rs.batch == batch && !rs.waited) { HIPCHK(hipStreamWaitEvent(st, rs.ready, 0)); rs.waited = true; } }
            r_fresh = fresh_nursery;
            ready_spins = 0;
        }
        return true;
    }

    // will round_finish wait for the device (an update that is not merely written down)?
    bool finish_may_wait() const
    {
        const bool upd = h_ctl->status == PC_ST_UPDATE || (h_ctl->upd_pending && h_ctl->status == PC_ST_RUNNING);
        return upd && pc_choose_update(plan, update_facts(1)).may_wait;
    }
    // what the round did, once its stamp is in; false: the loop is over
    bool round_finish()
    {
        unsigned &batch = r_batch; int &nursery_left = r_nursery_left; const bool fresh_nursery = r_fresh;
        (void)batch;
        {
            // A run whose last death exhausts a nursery AND triggers an update learns that it is over only from the next
            // launch (the kernels test more_samples_needed before a death, nested_sampling.F90:237): the nursery
            // generated in between was never touched and does not count.
            if (fresh_nursery && h_ctl->status == PC_ST_DONE && h_ctl->i_nursery == B) tm.batches--;
            nursery_left = h_ctl->i_nursery;
            tally_grades();
            tm.rounds++;
            // dead rows leave for the host at every update (a copy per round, ~350 KB, next to the one-CU contraction cost it
            // 6 us per launch: 72 against 66 us)
            if (h_ctl->status == PC_ST_UPDATE || (h_ctl->upd_pending && h_ctl->status == PC_ST_RUNNING)) {
                do_update(h_ctl->status != PC_ST_UPDATE); h_ctl->status = PC_ST_RUNNING; h_ctl->upd_pending = 0;
                // (every few updates: in step with other runs a copy request costs the one thread that drives them all ~10 us, and a run on its own
                //  finds the k_slice next to a copy as much longer as the copy lasts -- four copies of a run's thirty-one: 11.40 -> 11.33 ms, three A/B pairs.
                //  The copy is a kernel of the runtime's, and whatever runs beside it pays its whole length, not k_slice alone: with the event in front
                //  of do_update() the copy ran beside the update, no k_slice was long any more (39 of 396 -> 0, 105 -> 51 us) and the updates beside a
                //  copy took 111 us instead of 58 -- 10.68 -> 10.67 ms at this threshold, 10.60 -> 10.70 ms at 2 * nlive.  So it stays behind the
                //  update: profiles/dead_rows.json)
                if ((size_t)h_ctl->ndead >= h_dead_copied + 4 * (size_t)cfg.nlive) {
                if (!ev_apply) ev_apply = hpool().get_sync_event();
                HIPCHK(hipEventRecord(ev_apply, st));       // the dead rows of the rounds so far are in place behind this point
                stream_dead();
                }
            }
        }
        return true;
    }

    // kill-off, results; the code pchip_run returns
    // ---- the end of a run in two halves, so that runs in step can end together: end_a asks the device for everything (kill-off,
    //      moments, copies), end_b -- once the stream has been waited for -- makes the results.  end() = both, for a run on its own.
    struct EndState {
        double *hlive = nullptr; int *hcl = nullptr; double *d_pmax = nullptr, *h_part = nullptr, *h_zp = nullptr;
        int nc_end = 0, ncd_max = 0, pmD = 0, pm_nb = 0, pm_pw = 0; clk::time_point t2;
    } es;
    // A run in step that ends with several clusters: its kill-off is the general contraction kernel, one workgroup for ~4 ms
    // (BASELINE configs[2]: a thousand deaths one after the other), and on the cohort's stream the other runs' next round waited
    // behind it -- sixteen endings 70 ms of a 670 ms call.  It goes to the run's copy stream, behind everything the run has had.
    hipStream_t st_fin = nullptr; hipEvent_t ev_fin = nullptr;
    void end_a(bool fused_final = false)
    {
        if (co && !fused_final) co->flush();      // (fused: the caller has launched what was pending, and launches the kill-offs together)
        bool &sort_valid = r_sort_valid;
        es.t2 = clk::now();
        st_fin = st;
        if (co && fused_final && !pc_env().cohort_final_aside_off && st_copy && st_copy != st && h_ctl->ncluster > 1) {
            ev_fin = hpool().get_sync_event();
            HIPCHK(hipEventRecord(ev_fin, st));
            HIPCHK(hipStreamWaitEvent(st_copy, ev_fin, 0));
            st_fin = st_copy;
        }
        hipStream_t st = st_fin;                  // (what follows is this run's alone)
        // snapshot of the live set at termination, then nested_sampling.F90:381-384
        const int nT = S.nT;
        // (pinned buffers, copies in stream order in front of the kill-off: the host does not stop here)
        es.hlive = blocks.pin<double>((size_t)S.Ncap * nT); es.hcl = blocks.pin<int>(S.Ncap);
        // A run on its own that ends through k_final_par: the loop's dead rows that have not left yet and the live rows go to the copy
        // stream from here, beside the kill-off (which writes neither: S.live stays, everything below h_ctl->ndead is final), and not
        // in front of it and behind the host's wait for it.  live_cluster stays in front: the kill-off rewrites it.
        const bool tail_aside = !co && plan.par_ok && h_ctl->ncluster == 1 && st_copy && st_copy != st;
        if (tail_aside) {
            if (!ev_apply) ev_apply = hpool().get_sync_event();
            HIPCHK(hipEventRecord(ev_apply, st));
            HIPCHK(hipStreamWaitEvent(st_copy, ev_apply, 0));
            stream_dead();
            HIPCHK(hipMemcpyAsync(es.hlive, S.live, sizeof(double) * (size_t)S.Ncap * nT, hipMemcpyDeviceToHost, st_copy));
        } else
        HIPCHK(hipMemcpyAsync(es.hlive, S.live, sizeof(double) * (size_t)S.Ncap * nT, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(es.hcl, S.live_cluster, sizeof(int) * S.Ncap, hipMemcpyDeviceToHost, st));
        es.nc_end = h_ctl->ncluster;
        if (h_ctl->ncluster == 0) {
            // a finished run read back from its .resume file: nothing to kill
        } else if (plan.par_ok && h_ctl->ncluster == 1) {
            path[PCHIP_PATH_KILLOFF_PAR]++;
            if (co && sort_valid) { co->rec(rec_final(S)); if (!fused_final) co->flush(); }      // (fused: the caller launches the kill-off of all runs that end now, then calls end_a2)
            else {
            if (!sort_valid) (void)pc_launch_sort_live(&S, st);
            if (co) (void)pc_launch_final_par(&S, st);
            else (void)pc_launch_final_par_split(&S, st);      // (k_final_par without its row loop, k_final_rows behind it)
            }
        } else if (h_ctl->ncluster > 1 && pc_launch_killoff_cl(&S, h_ctl->ncluster, st) == 0) {      // (several clusters: the deaths in sorted order by one wavefront, pc_clus.hip)
            path[PCHIP_PATH_KILLOFF_CL]++;
        } else if (plan.fast_ok && h_ctl->ncluster == 1 && pc_launch_consume_fast(&S, 1, st) == 0) path[PCHIP_PATH_KILLOFF_FAST]++;
        else { path[PCHIP_PATH_KILLOFF_GENERAL]++; pc_launch_consume(&S, 1, (h_ctl->ncluster > 1 && !S.seq_mode) ? 1 : 0, st); }   // (the general kernel: four waves, a death's jobs side by side)
        if (!fused_final) end_a2();
    }
    void end_a2()
    {
        hipStream_t st = st_fin ? st_fin : this->st;
        // what the results need from the device is requested here, behind the kill-off and before the host waits for it: the
        // posterior moments of theta over the dead points (device reduction, fixed order; the kernels take the count from the
        // control block) and the evidences of the retired clusters -- one wait instead of four
        es.pmD = S.D + S.nDer; es.pm_nb = pc_post_blocks(); es.pm_pw = 3 * es.pmD + 1;   // theta and phi columns are contiguous in a row
        es.ncd_max = std::min(h_ctl->ncluster_dead + h_ctl->ncluster, S.maxc_dead);
        // (the partial sums go straight into pinned host memory, which the device addresses like its own: 180 KB over the
        //  link instead of a D2H copy request behind the kernel -- that request stalled its caller for 5-6 ms once per process,
        //  in the second or third run)
        es.d_pmax = blocks.dev<double>(2 * (size_t)es.pm_nb); es.h_part = blocks.pin<double>((size_t)es.pm_nb * es.pm_pw);
        es.h_zp = blocks.pin<double>(2 * (size_t)std::max(1, es.ncd_max));
        pc_launch_post_moments(&S, -1, es.d_pmax, es.h_part, st);
        if (es.ncd_max > 0) {
            HIPCHK(hipMemcpyAsync(es.h_zp, S.logZp_dead, sizeof(double) * es.ncd_max, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(es.h_zp + es.ncd_max, S.logZp2_dead, sizeof(double) * es.ncd_max, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipMemcpyAsync(h_ctl, S.ctl, sizeof(PcCtl), hipMemcpyDeviceToHost, st));       // (read_ctl without its wait: end_b's caller waits)
        if (ev_fin) HIPCHK(hipEventRecord(ev_fin, st));      // (a kill-off beside the cohort's stream: end_b's caller waits for this one too)
    }
    void end_wait_aside() { if (ev_fin) { HIPCHK(hipEventSynchronize(ev_fin)); hpool().put_sync_event(ev_fin); ev_fin = nullptr; } }
    int end(pchip_result *out) { end_a(); HIPCHK(hipStreamSynchronize(st)); end_wait_aside(); return end_b(out); }
    int end_b(pchip_result *out)
    {
        // (when something below throws, the five blocks of the end stage stay in the ledger: destroy() waits for the copy stream, on which hlive
        //  may still be on its way, before they go back)
        double *hlive = es.hlive; int *hcl = es.hcl; double *h_part = es.h_part, *h_zp = es.h_zp;
        const int nc_end = es.nc_end, ncd_max = es.ncd_max, pmD = es.pmD, pm_nb = es.pm_nb, pm_pw = es.pm_pw, nT = S.nT;
        const auto t0 = r_t0, t1 = r_t1; auto t2 = es.t2;
        HIPCHK(hipGetLastError());                    // a kernel that could not be launched must not go unnoticed
        nph_stale = false;
        kt.collect();
        if (cfg.boost_posterior != 0.0 && (cfg.posteriors || cfg.equals) && h_ctl->nphantom > 0) {
            // the last update_posteriors (nested_sampling.F90:386-390): every remaining phantom is below the last death
            pc_launch_clean(&S, h_ctl->nphantom, keep, blk, d_total, ph2, phL2, phC2, phU2, nullptr, st);
            collect_phantom_posteriors(h_ctl->nphantom);
        }
        call_dumper(1);
        write_resume();
        auto t3 = clk::now();
        tm.t_gen = std::chrono::duration<double>(t1 - t0).count();
        tm.t_loop = std::chrono::duration<double>(t2 - t1).count();
        tm.t_final = std::chrono::duration<double>(t3 - t2).count();
        tm.t_total = std::chrono::duration<double>(t3 - t0).count();
        // ---- results (calculate_logZ_estimate, run_time_info.f90:652-678)
        std::memset(out, 0, sizeof(*out));
        out->logZ = std::max(-PC_HUGE, 2 * h_ctl->logZ - 0.5 * h_ctl->logZ2);
        out->varlogZ = h_ctl->logZ2 - 2 * h_ctl->logZ;
        out->ndead = h_ctl->ndead; out->nlike = h_ctl->nlike; out->niter = h_ctl->niter;
        out->nlike_failed = h_ctl->nlike_failed; out->ncluster_peak = ncluster_peak; out->epoch_discard = S.epoch_discard;
        path[PCHIP_PATH_NN_FALLBACKS] = (long)h_ctl->nn_fallbacks; path[PCHIP_PATH_POOL_MODE] = S.pool; path[PCHIP_PATH_DEFER_UPDATE] = S.defer_update;
        path[PCHIP_PATH_SLICE_STEP] = step_note.shared;
        for (int k = 0; k < PCHIP_PATH_COUNT; ++k) out->path[k] = path[k];
        grade_counts(out->nlike_grade);
        out->ncluster = nc_end; out->ncluster_dead = h_ctl->ncluster_dead; out->nbatches = tm.batches;
        out->nrounds = tm.rounds; out->nupdates = tm.updates; out->nTotal = nT; out->batch = B;
        out->t_generate = tm.t_gen; out->t_loop = tm.t_loop; out->t_final = tm.t_final; out->t_total = tm.t_total;
        for (int k = 0; k < KT_N; ++k) { out->k_time_s[k] = kt.total_ms[k] * 1e-3; out->k_launches[k] = kt.launches[k]; }
        // developer counters (PC_DEBUG=2|3|4); the feedback setting keeps the reference's meaning (feedback.f90)
        const int dbg_lvl = pc_env().debug;
        if (dbg_lvl >= 3) std::fprintf(stderr, "polychord_hip dbg general: term %lld identify %lld kill+add %lld tail %lld cycles; %lld chains identified from the candidate lists, %lld of them fell back to the full search\n", h_ctl->gen_cyc[0], h_ctl->gen_cyc[1], h_ctl->gen_cyc[2], h_ctl->gen_cyc[3], h_ctl->nn_walks, h_ctl->nn_fallbacks);
        if (dbg_lvl == 4) std::fprintf(stderr, "polychord_hip dbg par: stage+search %lld rank-sort %lld accept %lld merge+slots %lld evidence %lld triggers %lld publish %lld cycles\n", h_ctl->dbg[0], h_ctl->dbg[1], h_ctl->dbg[2], h_ctl->dbg[3], h_ctl->dbg[4], h_ctl->dbg[5], h_ctl->dbg[6]);
        if (dbg_lvl == 4) std::fprintf(stderr, "polychord_hip dbg par: %lld evidence scans as pairs (terms beyond one scale)\n", h_ctl->dbg[7]);
        if (dbg_lvl == 4 && h_ctl->wave_cyc[0]) std::fprintf(stderr, "polychord_hip dbg clp (several clusters; the line above then reads: decisions | order of deaths + slots | counts + volumes | volume sum + step 0's phantoms | prefix sums + commit | waves 1-3 | write back | passes): wave 1 %lld wave 2 %lld wave 3 %lld phantom wave %lld cycles\n", h_ctl->wave_cyc[0], h_ctl->wave_cyc[1], h_ctl->wave_cyc[2], h_ctl->wave_cyc[3]);
        if (dbg_lvl == 2) std::fprintf(stderr, "polychord_hip dbg: loop cycles %lld passB %lld (%lld flushes) accept-steps %lld (%lld) ins-rescan %lld (%lld) reject-steps cycles %lld\n", h_ctl->dbg[0], h_ctl->dbg[1], h_ctl->dbg[4], h_ctl->dbg[2], h_ctl->dbg[3], h_ctl->dbg[5], h_ctl->dbg[6], h_ctl->dbg[7]);
        if ((size_t)h_ctl->ndead > h_dead_cap) {          // the dead array grew beyond the first estimate
            HIPCHK(hipStreamSynchronize(st_copy));
            blocks.release(h_dead); h_dead_cap = (size_t)h_ctl->ndead; h_dead = blocks.pin<double>(h_dead_cap * nT); h_dead_copied = 0;
        }
        stream_dead();
        out->dead = blocks.hand_over(h_dead); h_dead = nullptr;      // (the result's three arrays are pchip_result_free's from here on)
        out->logweights = blocks.hand_over(blocks.pin<double>(std::max(1, h_ctl->ndead)));
        HIPCHK(hipMemcpyAsync(out->logweights, S.dead_logw, sizeof(double) * h_ctl->ndead, hipMemcpyDeviceToHost, st_copy));
        out->entry = blocks.hand_over(blocks.pin<double>(std::max(1, h_ctl->ndead)));
        HIPCHK(hipMemcpyAsync(out->entry, S.dead_entry, sizeof(double) * h_ctl->ndead, hipMemcpyDeviceToHost, st_copy));
        int nl = 0;
        for (int s = 0; s < S.Ncap; ++s) nl += hcl[s] >= 0;
        out->nlive_final = nl;
        out->live = (double *)std::malloc(sizeof(double) * (size_t)std::max(1, nl) * nT);
        out->live_cluster = (int *)std::malloc(sizeof(int) * (size_t)std::max(1, nl));
        for (int s = 0, k = 0; s < S.Ncap; ++s) if (hcl[s] >= 0) out->live_cluster[k++] = hcl[s];      // (the rows: behind the copy stream's wait below)
        const int ncd = std::min(h_ctl->ncluster_dead, S.maxc_dead);
        out->nZp = ncd;
        out->logZp = (double *)std::malloc(sizeof(double) * std::max(1, ncd));
        out->varlogZp = (double *)std::malloc(sizeof(double) * std::max(1, ncd));
        if (ncd > ncd_max) engine_fail(PC_RC_DEVICE, "more retired clusters (%d) than the final stage could have left (%d)", ncd, ncd_max);
        for (int i = 0; i < ncd; ++i) { const double zp = h_zp[i], zp2 = h_zp[ncd_max + i]; out->logZp[i] = 2 * zp - 0.5 * zp2; out->varlogZp[i] = zp2 - 2 * zp; }
        blocks.release(es.h_zp);
        // posterior moments of theta from the dead points (requested above): sums about the pivot row p (k_post_moments),
        // mean = p + S1 / W, variance = S2 / W - (S1 / W)^2
        const int D = pmD, nb = pm_nb, pw = pm_pw;
        out->post_mean = (double *)std::calloc(D, sizeof(double)); out->post_var = (double *)std::calloc(D, sizeof(double));
        double sw = 0.0;
        for (int b = 0; b < nb; ++b) {
            sw += h_part[(size_t)b * pw + 2 * D];
            for (int d = 0; d < D; ++d) { out->post_mean[d] += h_part[(size_t)b * pw + d]; out->post_var[d] += h_part[(size_t)b * pw + D + d]; }
        }
        for (int d = 0; d < D; ++d) {
            const double dm = out->post_mean[d] / sw;
            out->post_mean[d] = h_part[2 * D + 1 + d] + dm;
            out->post_var[d] = std::max(0.0, out->post_var[d] / sw - dm * dm);
        }
        blocks.release(es.d_pmax); blocks.release(es.h_part);
        // settings.device_records: the lived records picked here, on the device that made them (what the exchange step of repeat-sharded
        // runs sends); their count comes back with the wait below
        long long *h_nrec = nullptr;
        if (cfg.device_records && h_ctl->ndead > 0) {
            const long long cap = h_ctl->ndead;
            double *blk_rec = (double *)pc_cache_dev_alloc(pc_records_block_bytes(cap, nT));
            if (!blk_rec) engine_fail(PC_RC_MEMORY, "no device memory for the run's records (%lld rows)", cap);
            h_nrec = blocks.pin<long long>(1);
            if (pc_pack_lived_device(S.dead, S.dead_logw, S.dead_entry, cap, nT, cfg.logzero, blk_rec, cap, h_nrec, st_copy) != 0) { pc_cache_dev_free(blk_rec); engine_fail(PC_RC_DEVICE, "packing the run's records"); }
            out->d_records = blk_rec; out->records_cap = (long)cap; out->records_device = dev;
        }
        HIPCHK(hipStreamSynchronize(st_copy));
        for (int s = 0, k = 0; s < S.Ncap; ++s) if (hcl[s] >= 0) std::memcpy(out->live + (size_t)(k++) * nT, hlive + (size_t)s * nT, sizeof(double) * nT);      // (a run on its own: the live rows came by the copy stream, end_a)
        if (h_nrec) { out->n_records = (long)*h_nrec; blocks.release(h_nrec); }
        blocks.release(es.hlive); blocks.release(es.hcl);
        active_run.reset();
        return 0;
    }

    // (streams_idle: the caller has waited for everything the run's streams were given -- a run in step whose ending was waited
    //  for by event; six stream waits from each of eight threads at once were half of the teardown's time)
    void destroy(bool streams_idle = false)
    {
        active_run.reset();
        // work may still be in flight on any of the run's streams (early returns, the prefetched bases of a nursery
        // that was never consumed): the blocks below go back to a process-wide cache and may be handed to another
        // run's thread at once
        if (!streams_idle) {
        if (st) (void)hipStreamSynchronize(st);
        if (st_copy) (void)hipStreamSynchronize(st_copy);
        if (st_side) (void)hipStreamSynchronize(st_side);
        }
        const auto dq0 = std::chrono::steady_clock::now();
        // every block the run still holds, whichever path allocated it and however the run ended (the staging blocks of a wait that never came,
        // the end stage's of an end_b that threw): the ledger knows them, this function names none
        blocks.release_all();
        fetching.clear(); own_fetches.clear(); staged_up.clear();
        h_dead = nullptr; h_ctl = nullptr; h_note = nullptr; es = EndState();
        const auto dq1 = std::chrono::steady_clock::now();
        kt.destroy();
        if (ev_apply) { hpool().put_sync_event(ev_apply); ev_apply = nullptr; }

        if (st) { if (!streams_idle) (void)hipStreamSynchronize(st); if (!co) hpool().put_stream(st); } st = nullptr;
        if (st_copy) { if (!streams_idle) (void)hipStreamSynchronize(st_copy); if (!st_copy_shared) hpool().put_stream(st_copy); } st_copy = nullptr;
        if (st_side) {
            if (!streams_idle) (void)hipStreamSynchronize(st_side); hpool().put_stream(st_side); hpool().put_sync_event(ev_main);
            if (ev_presort_a) { hpool().put_sync_event(ev_presort_a); hpool().put_sync_event(ev_presort_b); ev_presort_a = ev_presort_b = nullptr; }
            for (int r = 0; r < RAW_RING; ++r) { if (ring[r].ready) hpool().put_sync_event(ring[r].ready); if (ring[r].consumed) hpool().put_sync_event(ring[r].consumed); ring[r] = RawSlot(); }
        }
        st_side = nullptr; ev_main = nullptr;
        const auto dq2 = std::chrono::steady_clock::now();
        g_dbg_d1 += std::chrono::duration_cast<std::chrono::nanoseconds>(dq1 - dq0).count();
        g_dbg_d2 += std::chrono::duration_cast<std::chrono::nanoseconds>(dq2 - dq1).count();
    }
};

}  // namespace

#include "pc_tick.h"        // TickGroup: what the runs of a group share when their likelihood is the caller's device batch callback
#include "pc_step.h"        // pc_run_many: the driver of the runs in step, a group at a time, as named phases (StepGroup)
#include "pc_doors.h"       // the kernel-level doors of the tests (pchip_slice_chains ... pchip_cluster_update); door_guard, with_engine

extern "C" {

void polychord_hip_request_stop(void) { std::lock_guard<std::mutex> g(g_run_mutex); for (auto *f : g_run_stop) f->store(1); }
// tests of the error paths: the next run fails once at the chosen point (1: a device allocation, 2: the cluster
// capacity at the next split, 3: the phantom array at its next growth); 0 disarms
void pchip_inject_fault(int kind) { g_inject_fault = kind; }
// the block caches for the library's other files (the merge's scratch and its rows): null when there is no memory.  The merge
// took its scratch from the driver and gave it back at its end: the driver then works the frees off for 10 ... 30 ms, and the
// next call's first wait for the device -- if it came at once -- sat behind that
void *pc_cache_dev_alloc(size_t bytes) { try { return dcache().get(bytes); } catch (const EngineError &) { (void)hipGetLastError(); return nullptr; } }
void pc_cache_dev_free(void *p) { if (p && !dcache().put(p)) (void)hipFree(p); }
void *pc_cache_host_alloc(size_t bytes) { try { return hcache().get(bytes); } catch (const EngineError &) { (void)hipGetLastError(); return nullptr; } }
void pc_cache_host_free(void *p) { if (p && !hcache().put(p)) (void)hipHostFree(p); }
void pchip_blocks_in_use(long *device, long *pinned) { if (device) *device = dcache().in_use(); if (pinned) *pinned = hcache().in_use(); }
void pchip_trim_cache(void) { (void)hipDeviceSynchronize(); dcache().trim(); hcache().trim(); }      // the blocks finished runs left for the next ones go back to the driver
// initial capacity of the per-cluster arrays (default 128) and of the phantom array in rows (0 = the engine's estimate);
// both grow on demand, so these only matter to tests of the growth paths
void pchip_set_capacity(int clusters, int phantom_rows) { if (clusters > 0) g_cap_clusters = clusters; if (phantom_rows >= 0) g_cap_phantoms = phantom_rows; }   // negative: leave as is
void polychord_hip_set_batch_callback(polychord_batch_fn fn, void *user) { std::lock_guard<std::mutex> g(g_cb_mutex); g_batch_fn = fn; g_batch_user = user; }
void polychord_hip_set_device_batch_callback(polychord_device_batch_fn fn, void *user) { std::lock_guard<std::mutex> g(g_cb_mutex); g_dbatch_fn = fn; g_dbatch_user = user; }

double polychord_hip_keyed_uniform(unsigned seed, unsigned dom, unsigned shi, unsigned slo, unsigned idx)
{   // the engine's counter RNG on the host (same numbers as pc_dev.h pc_uniform)
    return h_uniform(seed, 0x504F4C59u, dom, shi, slo, idx);
}

void pchip_settings_default(pchip_settings *s, int nDims, int nDerived)
{   // defaults of the reference's C++ Settings (src/polychord/c_interface.cpp:6-39)
    std::memset(s, 0, sizeof(*s));
    s->nDims = nDims; s->nDerived = nDerived; s->nlive = 500; s->num_repeats = 5 * nDims; s->nprior = -1; s->nfail = -1;
    s->precision_criterion = 0.001; s->logzero = -1e30; s->max_ndead = -1; s->compression_factor = 0.36787944117144233;
    s->seed = -1; s->batch = 0; s->device = -1;
}

int pchip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pchip_run(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, pchip_result *out)
{
    return pchip_run_hooks(s, like, prior, nullptr, out);
}

int pchip_run_hooks(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, const pchip_hooks *hooks, pchip_result *out)
{
    if (s->num_repeats < 1) { std::fprintf(stderr, "polychord_hip: You need to set num_repeats. Suggestion: 5*nDims\n"); return 1; } // settings.f90:216
    if (s->num_repeats > 64 * PC_MASK_WORDS) { std::fprintf(stderr, "polychord_hip: num_repeats > %d unsupported\n", 64 * PC_MASK_WORDS); return 1; }
    if (like->kind == PC_LIKE_CALLBACK && !like->fn) { std::fprintf(stderr, "polychord_hip: callback likelihood without a function pointer\n"); return 1; }
    // (a batched quadratic form under a host prior or a source prior: refused before any device call)
    if (const char *why = pc_quad_batch_refusal("pchip_run", like, prior, nullptr)) { std::fprintf(stderr, "polychord_hip: %s\n", why); pc_abi_set_last_error(why); std::memset(out, 0, sizeof(*out)); return 1; }
    using clk = std::chrono::steady_clock;
    auto t0 = clk::now();
    std::memset(out, 0, sizeof(*out));
    Engine E;
    if (hooks) { E.dumper = hooks->dumper; E.on_update = hooks->on_update; E.hook_user = hooks->user; }
    int rc;
    auto t1 = t0, t2 = t0;
    try {
        E.setup(*s, *like, *prior);
        t1 = clk::now();
        rc = E.run(out);
        t2 = clk::now();
    } catch (const EngineError &e) {
        std::fprintf(stderr, "polychord_hip: %s\n", e.msg.c_str());
        (void)hipGetLastError();
        rc = e.code;
        pchip_result_free(out);
        t2 = clk::now();
    } catch (const std::bad_alloc &) {
        std::fprintf(stderr, "polychord_hip: out of host memory\n");
        rc = PC_RC_MEMORY;
        pchip_result_free(out);
        t2 = clk::now();
    } catch (...) {                       // thrown by a host hook (a binding's halt request): pass it on, resources released
        pchip_result_free(out);
        E.destroy();
        throw;
    }
    E.destroy();
    auto t3 = clk::now();
    if (rc == 0) {
        out->t_setup = std::chrono::duration<double>(t1 - t0).count();
        out->t_teardown = std::chrono::duration<double>(t3 - t2).count();
        out->t_results = std::chrono::duration<double>(t2 - t1).count() - out->t_total;
    }
    return rc;
}

void pchip_result_free(pchip_result *r)
{
    hfree(r->dead); hfree(r->logweights); hfree(r->entry); std::free(r->live); std::free(r->logZp); std::free(r->varlogZp);
    if (r->d_records) pc_cache_dev_free(r->d_records);
    std::free(r->post_mean); std::free(r->post_var); std::free(r->live_cluster);
    std::memset(r, 0, sizeof(*r));
}

// the batch callback that is registered now (polychord_hip_set_batch_callback): the doors put theirs in only where the caller has none
void pc_batch_callback_get(polychord_batch_fn *fn, void **user) { std::lock_guard<std::mutex> g(g_cb_mutex); if (fn) *fn = g_batch_fn; if (user) *user = g_batch_user; }
// a device batch callback is registered now (polychord_hip_set_device_batch_callback): a callback likelihood's table prior then stays a table
int pc_device_batch_registered(void) { std::lock_guard<std::mutex> g(g_cb_mutex); return g_dbatch_fn != nullptr; }


// ---- the device maximiser: `maximise = T` for problems that live wholly on the device (k_max_rank, k_maximise: pc_sample.hip) -----------
// One engine state serves every run (the runs of pchip_run_in_step share their problem): its set-up gives the likelihood, the prior and the
// source's data block as the sampling kernels take them.  Two launches whatever the number of runs: the candidate values of the posterior
// legs over all live rows, then one wavefront per leg and run.  The choice of simplex and the result struct are pc_maximise.hip's.
static int maximise_device_core(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nruns, const double *const *live,
                                const int *const *cluster, const int *nlive, const double *const *mean, long max_iter, pchip_maximum *out)
{
    if (out && nruns >= 1) std::memset(out, 0, sizeof(pchip_maximum) * (size_t)nruns);     // every return leaves results that pchip_maximum_free takes
    if (!s || !like || !prior || !out || nruns < 1) { pc_abi_set_last_error("pchip_maximise_device: settings, likelihood, prior, at least one run and a result for each"); return 1; }
    if (like->kind == PC_LIKE_CALLBACK || prior->kind == PCHIP_PRIOR_CALLBACK) {
        pc_abi_set_last_error("pchip_maximise_device: a host callback likelihood or a host prior (kind 0) has no device code -- pchip_maximise / pchip_maximise_values polish through the host functions");
        return 1;
    }
    // (a batched quadratic form has no in-kernel evaluation for k_maximise to call: not covered)
    if (const char *why = pc_quad_batch_refusal("pchip_maximise_device", like, prior, nullptr)) { pc_abi_set_last_error(why); return 1; }
    const int D = s->nDims, nDer = s->nDerived, nT = 2 * D + nDer + 2, nv = D + 1;
    for (int r = 0; r < nruns; ++r)
        if (!live[r] || !cluster[r] || nlive[r] < 1) { pc_abi_set_last_error("pchip_maximise_device: every run needs its live rows, their clusters and nlive >= 1"); return 1; }
    if (D < 1 || nDer < 0) { pc_abi_set_last_error("pchip_maximise_device: nDims >= 1, nDerived >= 0"); return 1; }
    if (D > 64) { pc_abi_set_last_error("pchip_maximise_device: nDims > 64 is not supported (one coordinate a lane); the host maximiser remains for host functions"); return 3; }
    for (int r = 0; r < nruns; ++r) pc_maximum_alloc(&out[r], D, nDer);
    const size_t nin = (size_t)nv * D + nv + D + nDer, nout = (size_t)2 * D + 2 * nDer + 4;
    // the likelihood legs' simplexes need no device: a live set without one launches nothing
    std::vector<double> in; std::vector<int> hdr, prob_run, prob_leg;
    auto add_problem = [&](int r, int leg, const double *vals) {
        std::vector<double> rec(nin, 0.0);
        out[r].cluster[leg] = pc_max_choose_simplex(D, nT, s->logzero, live[r], cluster[r], nlive[r], vals, rec.data(), rec.data() + (size_t)nv * D);
        if (out[r].cluster[leg] < 0) { out[r].status[leg] = 1; return; }
        if (mean[r]) std::copy(mean[r], mean[r] + D + nDer, rec.begin() + (size_t)nv * D + nv);
        in.insert(in.end(), rec.begin(), rec.end());
        hdr.push_back(leg); hdr.push_back(mean[r] ? 1 : 0);
        prob_run.push_back(r); prob_leg.push_back(leg);
    };
    std::vector<char> rank_run(nruns, 0);
    long rows_total = 0;
    for (int r = 0; r < nruns; ++r) {
        add_problem(r, 0, nullptr);
        // a run whose likelihood leg has no simplex stops there, as pchip_maximise_values does: its posterior leg is not tried
        rank_run[r] = out[r].status[0] == 0;
        if (rank_run[r]) rows_total += nlive[r]; else { out[r].status[1] = 1; out[r].cluster[1] = -1; }
    }
    int rc = 0;
    if (rows_total > 0 || !prob_run.empty()) {
        pchip_settings c;
        pchip_settings_default(&c, D, nDer);
        c.nlive = 8; c.nprior = 8; c.batch = 1; c.num_repeats = 1; c.do_clustering = 0; c.seed = 1; c.feedback = 0;
        c.device = s->device; c.ablate = s->ablate; c.logzero = s->logzero;
        // (every block from the engine's ledger: its teardown gives them back, however this ends)
        rc = with_engine(c, *like, *prior, [&](Engine &E) {
            HIPCHK(hipStreamSynchronize(E.st));
            const PcState &S = E.S;
            if (rows_total > 0) {
                std::vector<double> rows((size_t)rows_total * nT), val((size_t)rows_total);
                size_t at = 0;
                for (int r = 0; r < nruns; ++r) if (rank_run[r]) { std::copy(live[r], live[r] + (size_t)nlive[r] * nT, rows.begin() + at * nT); at += nlive[r]; }
                double *d_rows = E.blocks.dev<double>(rows.size()), *d_val = E.blocks.dev<double>(val.size());
                HIPCHK(hipMemcpy(d_rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
                if (pc_launch_max_rank(&S, (int)rows_total, d_rows, d_val, E.st)) {
                    if (pc_rtc_error()) pc_abi_set_last_error(pc_rtc_error());
                    engine_fail(PC_RC_SETTINGS, "pchip_maximise_device: k_max_rank could not be launched (%s)", polychord_hip_last_error() ? polychord_hip_last_error() : "no such kernel");
                }
                HIPCHK(hipStreamSynchronize(E.st));
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpy(val.data(), d_val, sizeof(double) * val.size(), hipMemcpyDeviceToHost));
                at = 0;
                for (int r = 0; r < nruns; ++r) if (rank_run[r]) { add_problem(r, 1, val.data() + at); at += nlive[r]; }
            }
            const int np = (int)prob_run.size();
            if (np > 0) {
                std::vector<double> res((size_t)np * nout); std::vector<long long> resi((size_t)np * 2);
                double *d_in = E.blocks.dev<double>(in.size()), *d_out = E.blocks.dev<double>(res.size());
                int *d_hdr = E.blocks.dev<int>(hdr.size()); long long *d_outi = E.blocks.dev<long long>(resi.size());
                HIPCHK(hipMemcpy(d_in, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(d_hdr, hdr.data(), sizeof(int) * hdr.size(), hipMemcpyHostToDevice));
                if (pc_launch_maximise(&S, np, d_in, d_hdr, max_iter > 0 ? (long long)max_iter : 200000LL, d_out, d_outi, E.st)) {
                    if (pc_rtc_error()) pc_abi_set_last_error(pc_rtc_error());
                    engine_fail(PC_RC_SETTINGS, "pchip_maximise_device: k_maximise could not be launched (%s)", polychord_hip_last_error() ? polychord_hip_last_error() : "no such kernel");
                }
                HIPCHK(hipStreamSynchronize(E.st));
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpy(res.data(), d_out, sizeof(double) * res.size(), hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(resi.data(), d_outi, sizeof(long long) * resi.size(), hipMemcpyDeviceToHost));
                for (int p = 0; p < np; ++p) {
                    pchip_maximum &m = out[prob_run[p]];
                    const int leg = prob_leg[p];
                    const double *row = res.data() + (size_t)p * nout, *tail = row + 2 * D + nDer;
                    m.niter[leg] = (long)resi[2 * (size_t)p]; m.neval[leg] = (long)resi[2 * (size_t)p + 1];
                    if (leg == 0) {
                        m.max_logl = tail[0];
                        std::copy(row + D, row + 2 * D + nDer, m.max_point);
                        if (mean[prob_run[p]]) {                     // [mean theta | phi(mean theta)], as loglikelihood(mean) leaves it (maximiser.F90:77-80)
                            m.has_mean = 1; m.logl_mean = tail[2];
                            std::copy(mean[prob_run[p]], mean[prob_run[p]] + D, m.mean_point);
                            std::copy(tail + 4, tail + 4 + nDer, m.mean_point + D);
                        }
                    } else {
                        m.logl_at_post = tail[0]; m.max_post = tail[0] + tail[1];
                        std::copy(row + D, row + 2 * D + nDer, m.post_point);
                    }
                }
            }
            return 0;
        }, true);      // (the message into polychord_hip_last_error() too; an error without a code is PC_RC_DEVICE)
    }
    if (rc) { for (int r = 0; r < nruns; ++r) pchip_maximum_free(&out[r]); return rc; }
    for (int r = 0; r < nruns; ++r)
        if (out[r].status[0] || out[r].status[1]) { pc_abi_set_last_error("pchip_maximise_device: Could not construct simplex (no cluster of the live set holds nDims + 1 rows above logzero)"); rc = 1; }
    return rc;
}

int pchip_maximise_device(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, const double *live, const int *live_cluster,
                          int nlive, const double *post_mean, long max_iter, pchip_maximum *out)
{
    return maximise_device_core(s, like, prior, 1, &live, &live_cluster, &nlive, &post_mean, max_iter, out);
}

int pchip_maximise_device_many(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, int nruns, const pchip_result *runs,
                               long max_iter, pchip_maximum *out)
{
    if (out && nruns >= 1) std::memset(out, 0, sizeof(pchip_maximum) * (size_t)nruns);
    if (!runs || nruns < 1) { pc_abi_set_last_error("pchip_maximise_device_many: at least one run"); return 1; }
    std::vector<const double *> live(nruns), mean(nruns); std::vector<const int *> cl(nruns); std::vector<int> nl(nruns);
    for (int r = 0; r < nruns; ++r) { live[r] = runs[r].live; cl[r] = runs[r].live_cluster; nl[r] = runs[r].nlive_final; mean[r] = runs[r].post_mean; }
    return maximise_device_core(s, like, prior, nruns, live.data(), cl.data(), nl.data(), mean.data(), max_iter, out);
}

}  // extern "C"
