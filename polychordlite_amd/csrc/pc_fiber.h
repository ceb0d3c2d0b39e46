// pc_fiber.h -- a run's host work that has to WAIT for the device in the middle, as a fiber of the thread that drives the runs in step.
//
// Included by pc_engine.hip ahead of Engine (and by tools/dev/step_record.hip), inside the including file's anonymous namespace, as pc_cohort.h
// is: the system headers named below must have been included at file scope before, so that here they are no-ops (both includers do).  The
// including file also provides the HIP stream calls and HIPCHK, which pc_wait_stream at the foot uses: it is here because Engine::sync_point,
// ahead of pc_step.h, and the driver's shared wait both need it.
//
// An update with clustering sends counts down, reads verdicts back, splits.  Where a run on its own synchronises its stream, a run in step
// yields (Engine::sync_point); the driver (pc_step.h) goes through all the runs that have something to wait for, launches what they wrote
// down ONCE for all of them, waits ONCE, and resumes them.  The waits of sixteen runs' updates cost what one run's do, and the kernels between
// two waits are launched together.  (makecontext / swapcontext: no threads, no locks; an exception inside a fiber is caught at its foot and
// rethrown by the driver.)
#pragma once
#include <ucontext.h>
#include <sys/mman.h>
#include <unistd.h>
#include <cstdint>
#include <new>
#include <functional>
#include <exception>

struct FiberCancelled {};      // thrown inside a suspended fiber that is resumed only to unwind (another run's update failed)
struct Fiber {
    ucontext_t ctx, ret;
    void *stack = nullptr; size_t stack_sz = 0;      // usable part; one PROT_NONE page below it (stacks grow down): an overflow faults
    void *map = nullptr; size_t map_sz = 0;          // instead of running into the heap
    std::function<void()> fn;
    bool started = false, done = false, cancel = false;
    std::exception_ptr err;
    // round_finish with clustering goes deep (update, kNN passes, add_cluster, the resume file's writer, HIP runtime calls): 8 MB of
    // address space, committed as touched
    void make_stack()
    {
        if (stack) return;
        const size_t page = (size_t)sysconf(_SC_PAGESIZE), want = (size_t)8 << 20;
        void *m = mmap(nullptr, want + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_STACK, -1, 0);
        if (m == MAP_FAILED) throw std::bad_alloc();
        (void)mprotect(m, page, PROT_NONE);
        map = m; map_sz = want + page; stack = (char *)m + page; stack_sz = want;
    }
    void free_stack() { if (map) munmap(map, map_sz); map = stack = nullptr; map_sz = stack_sz = 0; }
    static void foot(unsigned lo, unsigned hi)
    {
        Fiber *f = (Fiber *)(((uintptr_t)hi << 32) | (uintptr_t)lo);
        try { f->fn(); } catch (...) { f->err = std::current_exception(); }
        f->done = true;
        swapcontext(&f->ctx, &f->ret);
    }
    void resume()
    {
        if (!started) {
            getcontext(&ctx);
            ctx.uc_stack.ss_sp = stack; ctx.uc_stack.ss_size = stack_sz; ctx.uc_link = nullptr;
            const uintptr_t a = (uintptr_t)this;
            makecontext(&ctx, (void (*)())foot, 2, (unsigned)(a & 0xFFFFFFFFu), (unsigned)(a >> 32));
            started = true;
        }
        swapcontext(&ret, &ctx);
    }
    void yield() { swapcontext(&ctx, &ret); }
};

// the wait of a thread that has nothing else to do: polling the stream wakes the host a few microseconds after the work is done, the
// blocking wait sleeps on an interrupt -- so poll for a while first
inline void pc_wait_stream(hipStream_t st)
{
    for (int spins = 0; spins < 200000; ++spins) { const hipError_t q = hipStreamQuery(st); if (q != hipErrorNotReady) { HIPCHK(q); break; } __builtin_ia32_pause(); }
    HIPCHK(hipStreamSynchronize(st));
}
