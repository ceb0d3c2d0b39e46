// pc_blocks.h -- who owns a run's device and pinned blocks: the process-wide caches they come from and go back to, and the ledger a run keeps
// of the blocks it holds, from which its teardown releases them.
//
// Host only.  Included by pc_engine.hip alone, inside its namespace, in front of everything that allocates.  The top half (the caches and the
// four primitives dalloc / dfree / halloc / hfree) needs of the including file: HIP, engine_fail and PC_RC_MEMORY, g_inject_fault, pc_env()
// (pc_plan.h) and the g_dbg_miss_* counters.  The bottom half, RunBlocks, is written against the four primitive names alone -- and, for regrow,
//   dcopy_wait(dst, src, bytes, stream)      a device-to-device copy on the stream and the host's wait for it
// A file that defines PC_BLOCKS_OWN_PRIMITIVES first gets the ledger alone, over primitives of its own (tools/dev: the recorders, blocks_record.cpp).
#pragma once
#include <vector>
#include <cstddef>
#ifndef PC_BLOCKS_OWN_PRIMITIVES
// Process-wide cache of device blocks and pinned host blocks.  A run allocates ~70 buffers; hipMalloc /
// hipFree cost O(100 us) each and hipFree synchronises the device, which is as long as the sampling
// itself at the metric config.  Blocks are keyed by (device, rounded size) and handed back on free;
// nothing relies on their contents (hipMalloc does not zero either).
struct BlockCache {
    std::mutex m;
    std::multimap<std::pair<int, size_t>, void *> free_;
    std::unordered_map<void *, std::pair<int, size_t>> owner;
    size_t cached = 0, limit;
    bool host;
    BlockCache(bool h, size_t lim) : limit(lim), host(h) {}
    // eight sizes per octave above 4 KB (at most an eighth more than asked for): arrays sized by what a run found -- its dead
    // points, its weights -- differ by a few rows from seed to seed, and every near miss was a trip to the driver (a pinned
    // allocation is milliseconds there once another runtime, PyTorch's, lives in the process)
    static size_t round_up(size_t b)
    {
        if (b < 4096) return (b + 255) & ~(size_t)255;
        int top = 63 - __builtin_clzll((unsigned long long)b);
        const size_t step = (size_t)1 << (top - 3);
        return (b + step - 1) & ~(step - 1);
    }
    void *get(size_t bytes)
    {
        int dev = 0;
        if (!host) (void)hipGetDevice(&dev);
        const size_t sz = round_up(bytes ? bytes : 1);
        if (!host && sz >= (256u << 10) && g_inject_fault.load() == 1) { g_inject_fault = 0; engine_fail(PC_RC_MEMORY, "out of device memory (%zu bytes): injected", sz); }
        {
            std::lock_guard<std::mutex> g(m);
            auto it = free_.find({dev, sz});
            if (it != free_.end()) { void *p = it->second; free_.erase(it); cached -= sz; return p; }
        }
        void *p = nullptr;
        const auto q0 = std::chrono::steady_clock::now();
        hipError_t e = host ? hipHostMalloc(&p, sz) : hipMalloc(&p, sz);
        g_dbg_miss_n[host ? 1 : 0]++; g_dbg_miss_ns[host ? 1 : 0] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - q0).count();
        if (e != hipSuccess) {          // give the cached blocks back and retry once
            trim();
            e = host ? hipHostMalloc(&p, sz) : hipMalloc(&p, sz);
        }
        if (e != hipSuccess) { (void)hipGetLastError(); engine_fail(PC_RC_MEMORY, "out of %s memory (%zu bytes): %s", host ? "pinned host" : "device", sz, hipGetErrorString(e)); }
        std::lock_guard<std::mutex> g(m);
        owner[p] = {dev, sz};
        return p;
    }
    bool put(void *p)                   // false: not one of ours
    {
        {
            std::lock_guard<std::mutex> g(m);
            auto it = owner.find(p);
            if (it == owner.end()) return false;
            if (cached + it->second.second <= limit) { free_.insert({it->second, p}); cached += it->second.second; return true; }
            owner.erase(it);
        }
        if (host) (void)hipHostFree(p); else (void)hipFree(p);      // (over the limit: back to the driver, and not under the lock)
        return true;
    }
    // a run's hundred-odd blocks at its end in one visit: eight threads tearing runs down at once spent most of that time queueing
    // for the lock, block by block
    void put_many(const std::vector<void *> &ps)
    {
        std::vector<void *> over;
        {
            std::lock_guard<std::mutex> g(m);
            for (void *p : ps) {
                auto it = owner.find(p);
                if (it == owner.end()) continue;
                if (cached + it->second.second <= limit) { free_.insert({it->second, p}); cached += it->second.second; }
                else { owner.erase(it); over.push_back(p); }
            }
        }
        for (void *p : over) { if (host) (void)hipHostFree(p); else (void)hipFree(p); }
    }
    void trim()
    {
        std::lock_guard<std::mutex> g(m);
        for (auto &kv : free_) { if (host) (void)hipHostFree(kv.second); else (void)hipFree(kv.second); owner.erase(kv.second); }
        free_.clear(); cached = 0;
    }
    long in_use() { std::lock_guard<std::mutex> g(m); return (long)owner.size() - (long)free_.size(); }      // (obtained from the driver and held by somebody now: pchip_blocks_in_use)
};
// never destroyed: the HIP runtime may already be gone when static destructors run
BlockCache &dcache() { static BlockCache *c = new BlockCache(false, (size_t)64 << 30); return *c; }
BlockCache &hcache() { static BlockCache *c = new BlockCache(true, (size_t)12 << 30); return *c; }

// PC_POISON=1 (tests): every device block is filled with 0x5A bytes when it is handed out -- ints become 1515870810,
// doubles 2.6e127 -- so that a buffer some path forgets to initialise fails loudly instead of working by the luck of
// what the previous run left in it
template <class T> T *dalloc(size_t n)
{
    T *p = (T *)dcache().get(sizeof(T) * (n ? n : 1));
    if (pc_env().poison) { (void)hipMemset((void *)p, 0x5A, sizeof(T) * (n ? n : 1)); (void)hipDeviceSynchronize(); }
    return p;
}
template <class T> void dfree(T *&p) { if (p) dcache().put((void *)p); p = nullptr; }
void dfree(const std::vector<void *> &ps) { dcache().put_many(ps); }      // (a teardown's blocks in one visit to the lock)
template <class T> T *halloc(size_t n) { return (T *)hcache().get(sizeof(T) * (n ? n : 1)); }
void hfree(void *p) { if (p && !hcache().put(p)) std::free(p); }
void dcopy_wait(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
}
#endif

// The blocks a run holds, in the order it obtained them.  Every buffer of a run is allocated through its ledger, so one line -- the
// allocation -- is all a new buffer needs: whatever is still written down when the run ends, however it ends, goes back in release_all().
// The destructor releases nothing: a block must not return to the process-wide cache while work on it is in flight, and only the
// owner (Engine::destroy) knows when the run's streams have been waited for.
struct RunBlocks {
    struct Entry { void *p; bool pinned; };
    std::vector<Entry> held;
    template <class T> T *dev(size_t n) { room(); T *p = dalloc<T>(n); held.push_back({(void *)p, false}); return p; }
    template <class T> T *pin(size_t n) { room(); T *p = halloc<T>(n); held.push_back({(void *)p, true}); return p; }
    // one block back now (the grow paths, the transient staging blocks); null, or a block that is not written down here: nothing goes back
    template <class T> void release(T *&p)
    {
        void *q = (void *)p; bool pinned = false; p = nullptr;
        if (!forget(q, &pinned)) return;
        if (pinned) hfree(q); else dfree(q);
    }
    // a block of n in p's place with p's first `keep` elements, copied on the stream and waited for; the old block goes back
    template <class T, class Stream> void regrow(T *&p, size_t n, size_t keep, Stream st)
    {
        T *q = dev<T>(n);
        dcopy_wait((void *)q, (const void *)p, sizeof(T) * keep, st);
        release(p); p = q;
    }
    // the block is somebody else's to release from now on (a result's arrays: pchip_result_free)
    template <class T> T *hand_over(T *p) { forget((void *)p); return p; }
    // everything still written down, in allocation order; the device blocks in one visit to their cache's lock
    void release_all()
    {
        std::vector<void *> d; d.reserve(held.size());
        for (const Entry &e : held) { if (e.pinned) hfree(e.p); else d.push_back(e.p); }
        held.clear();
        dfree(d);
    }
private:
    void room() { if (held.size() == held.capacity()) held.reserve(2 * held.size() + 64); }      // (before the allocation: writing it down cannot fail)
    bool forget(const void *q, bool *pinned = nullptr)      // (looked for from the youngest: the transient ones)
    {
        if (q) for (size_t i = held.size(); i-- > 0;) if (held[i].p == q) { if (pinned) *pinned = held[i].pinned; held.erase(held.begin() + (std::ptrdiff_t)i); return true; }
        return false;
    }
};
