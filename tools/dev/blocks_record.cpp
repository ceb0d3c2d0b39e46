// blocks_record.cpp -- the rules of a run's ledger of blocks (RunBlocks, polychordlite_amd/csrc/pc_blocks.h), checked on the CPU.
//
// Plain C++, no HIP: the ledger over malloc-backed primitives that count what is out, which kind it is and how often the device cache's lock
// would have been visited.  A block released twice, or written to after its release, is the address sanitizer's to find; a block never released
// is the counters' (and the leak checker's).  Exit code 0 and a summary line when every scenario holds; 1 and the scenarios that do not otherwise.
// Built with the address and undefined-behaviour sanitizers (make -C polychordlite_amd/csrc blocks_record); tests/test_run_blocks.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace rec {
std::map<void *, bool> out;             // the blocks that are out: block -> pinned
long many_calls = 0;                    // visits to the device cache's lock by a release of many
long count(bool pinned) { long n = 0; for (auto &kv : out) n += kv.second == pinned; return n; }
void *get(size_t bytes, bool pinned) { void *p = std::malloc(bytes ? bytes : 1); out[p] = pinned; return p; }
void put(void *p, bool pinned)
{
    auto it = out.find(p);
    if (it == out.end() || it->second != pinned) { std::fprintf(stderr, "a block went back that is not out, or to the other cache\n"); std::abort(); }
    out.erase(it); std::free(p);
}
}
template <class T> T *dalloc(size_t n) { return (T *)rec::get(sizeof(T) * n, false); }
template <class T> void dfree(T *&p) { if (p) rec::put((void *)p, false); p = nullptr; }
void dfree(const std::vector<void *> &ps) { rec::many_calls++; for (void *p : ps) rec::put(p, false); }
template <class T> T *halloc(size_t n) { return (T *)rec::get(sizeof(T) * n, true); }
void hfree(void *p) { if (p) rec::put(p, true); }
long copies = 0;
void dcopy_wait(void *dst, const void *src, size_t bytes, int /* stream */) { if (bytes) std::memcpy(dst, src, bytes); copies++; }

#define PC_BLOCKS_OWN_PRIMITIVES
#include "pc_blocks.h"

static int failed = 0, scenarios = 0;
static void check(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); failed++; } }
static long dev_out() { return rec::count(false); }
static long pin_out() { return rec::count(true); }

int main()
{
    {   // allocate, release all: in allocation order, the device blocks in one visit
        scenarios++;
        RunBlocks b; rec::many_calls = 0;
        double *a = b.dev<double>(10); int *c = b.pin<int>(4); char *d = b.dev<char>(0); unsigned *e = b.pin<unsigned>(7);
        a[9] = 1.0; c[3] = 2; d[0] = 3; e[6] = 4u;
        check(dev_out() == 2 && pin_out() == 2 && b.held.size() == 4, "four blocks out, two of each kind");
        check(b.held[0].p == a && b.held[1].p == c && b.held[2].p == d && b.held[3].p == e && !b.held[0].pinned && b.held[1].pinned, "entries in allocation order, each with its kind");
        b.release_all();
        check(dev_out() == 0 && pin_out() == 0 && b.held.empty() && rec::many_calls == 1, "release-all leaves nothing out, with one visit to the device cache");
    }
    {   // release one in the middle, then all: no double release (put() aborts on one)
        scenarios++;
        RunBlocks b;
        double *a = b.dev<double>(3); double *m = b.pin<double>(5); int *z = b.dev<int>(2);
        b.release(m);
        check(m == nullptr && pin_out() == 0 && dev_out() == 2 && b.held.size() == 2 && b.held[0].p == a && b.held[1].p == z, "the middle block went back and the others kept their order");
        b.release(m);                                           // null: nothing
        int local = 0, *stranger = &local; b.release(stranger);   // not written down here: nothing goes back
        check(dev_out() == 2 && b.held.size() == 2, "a null pointer and a stranger release nothing");
        b.release_all();
        check(dev_out() == 0 && pin_out() == 0, "release-all after a release of one");
    }
    {   // regrow keeps the first `keep` elements and releases the old block
        scenarios++;
        RunBlocks b; copies = 0;
        int *p = b.dev<int>(8); double *other = b.dev<double>(1);
        for (int i = 0; i < 8; ++i) p[i] = 100 + i;
        int *old = p;
        b.regrow(p, 32, 5, 0);
        bool same = true; for (int i = 0; i < 5; ++i) same = same && p[i] == 100 + i;
        p[31] = 7;
        check(same && copies == 1 && dev_out() == 2 && b.held.size() == 2 && rec::out.count(old) == 0, "regrow: the first five kept, one copy, the old block back");
        check(b.held[0].p == other && b.held[1].p == p, "regrow: the new block is the youngest entry");
        b.regrow(p, 64, 0, 0);
        check(dev_out() == 2 && b.held.size() == 2, "regrow with nothing to keep");
        b.release_all();
        check(dev_out() == 0, "release-all after regrow");
    }
    {   // hand-over leaves the block alive after release-all, and the caller frees it
        scenarios++;
        RunBlocks b;
        double *dead = b.pin<double>(6); int *x = b.dev<int>(1);
        double *given = b.hand_over(dead);
        double *fresh = b.hand_over(b.pin<double>(3));
        check(given == dead && b.held.size() == 1 && b.held[0].p == x, "hand-over forgets the block");
        b.release_all();
        check(pin_out() == 2 && dev_out() == 0, "the blocks handed over outlive release-all");
        given[5] = 1.0; fresh[2] = 2.0;
        hfree(given); hfree(fresh);
        check(pin_out() == 0, "their new owner frees them");
    }
    {   // an exception between two allocations, caught outside, then release-all
        scenarios++;
        RunBlocks b;
        try {
            double *rows = b.dev<double>(12); int *h = b.pin<int>(2);
            rows[0] = 1.0; h[0] = 1;
            throw std::runtime_error("the host likelihood raised");
            double *never = b.dev<double>(12); (void)never;
        } catch (const std::runtime_error &) {}
        check(dev_out() == 1 && pin_out() == 1 && b.held.size() == 2, "the blocks of the frames that unwound are still written down");
        b.release_all();
        check(dev_out() == 0 && pin_out() == 0, "release-all after an exception leaves nothing out");
    }
    {   // release-all twice is harmless
        scenarios++;
        RunBlocks b;
        (void)b.dev<int>(3); (void)b.pin<int>(3);
        b.release_all(); b.release_all();
        check(dev_out() == 0 && pin_out() == 0 && b.held.empty(), "release-all twice");
        int *again = b.dev<int>(1);
        check(b.held.size() == 1 && b.held[0].p == again, "the ledger serves after a release-all");
        b.release_all();
    }
    {   // 10 000 transient pairs leave the ledger no larger than it began: the staging path cannot grow it
        scenarios++;
        RunBlocks b;
        for (int i = 0; i < 100; ++i) (void)b.dev<double>(4);
        const size_t n0 = b.held.size(), cap0 = b.held.capacity();
        for (int i = 0; i < 10000; ++i) {
            void *h = b.pin<char>(64 + (size_t)i % 7), *g = b.pin<char>(16);
            std::memset(h, i & 0xFF, 64);
            b.release(h); b.release(g);
        }
        check(b.held.size() == n0 && b.held.capacity() == cap0 && pin_out() == 0 && dev_out() == 100, "10000 transient pairs: the ledger's length and room are what they were");
        b.release_all();
        check(dev_out() == 0, "release-all after the transient pairs");
    }
    {   // the destructor releases nothing: only the owner knows when the streams have been waited for
        scenarios++;
        double *p = nullptr;
        { RunBlocks b; p = b.dev<double>(2); }
        check(dev_out() == 1, "a ledger that goes out of scope releases nothing");
        dfree(p);
    }
    std::printf("%d scenarios, %d checks failed\n", scenarios, failed);
    return failed ? 1 : 0;
}
