// cohort_record.hip -- what the cohort of the runs in step (pc_cohort.h) launches, waits for and uploads, recorded on the CPU.
//
// Includes pc_cohort.h with recorders standing in for the launchers of pc_launch.h that it calls (another one fails to link here: add its
// recorder), for the HIP stream, event and copy calls, and for the services the header asks of its including file; then writes fabricated
// records down and flushes them, scenario by scenario, from a fixed-seed generator.  No device, no kernel runs.  Built host-only
// (make -C polychordlite_amd/csrc cohort_record); tests/test_cohort_record.py compares the digests with those of the Cohort of the commit
// before the table of stages (abd2406).
//
//   cohort_record            one line per scenario: its name, the digest of its record, the number of lines
//   cohort_record --dump     the records themselves
// With -DCOHORT_PARENT='"FILE"' (make cohort_record_parent COHORT_PARENT='"FILE"': its own binary, cohort_record_parent) the same scenarios
// drive FILE instead: lines 493-676 of abd2406's pc_engine.hip (its CK_* enum and Cohort),
// written down by the brace lists of that commit's call sites -- the adapters w_*() below hold both spellings.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <vector>
#include <array>
#include <functional>
#include <algorithm>
#include <initializer_list>
#include "pc_state.h"
#include "pc_launch.h"

struct Cohort;
namespace rec {
std::string text;                          // the record of the scenario in progress
Cohort *cur = nullptr;
const PcManyRec *dev_block = nullptr;      // where the last upload went
const char *decline = nullptr;             // the _many launcher that answers "not this way" ("*": all of them)
void line(const std::string &s) { text += s; text += '\n'; }
std::string num(long long v) { return std::to_string(v); }
std::string stream(hipStream_t q);
std::string event(hipEvent_t e);
hipError_t event_record(hipEvent_t e, hipStream_t q) { line("record " + event(e) + " on " + stream(q)); return hipSuccess; }
hipError_t stream_wait(hipStream_t q, hipEvent_t e) { line("wait " + event(e) + " on " + stream(q)); return hipSuccess; }
hipError_t event_sync(hipEvent_t e) { line("host waits " + event(e)); return hipSuccess; }
hipError_t upload(void *dst, const void *src, size_t bytes, hipStream_t q)
{
    std::memcpy(dst, src, bytes);
    dev_block = (const PcManyRec *)dst;
    const PcManyRec *r = (const PcManyRec *)src;
    std::string s = "upload on " + stream(q) + ":";
    for (size_t i = 0; i < bytes / sizeof(PcManyRec); ++i) {
        s += " [run " + num(r[i].S.src_pad) + " p";
        for (void *p : r[i].p) s += " " + num((long long)(uintptr_t)p);
        s += " ia";
        for (int v : r[i].ia) s += " " + num(v);
        s += "]";
    }
    line(s);
    return hipSuccess;
}
// a launcher's call: its name (where: the records of a launch for several runs), the run whose state it was given (-1: none), its other
// arguments, its stream; a launcher for several runs declines when it is the one named in `decline`
int launch(const char *name, const std::string &where, const PcState *S, std::initializer_list<long long> args, hipStream_t q)
{
    std::string s = std::string("launch ") + name + where + " run " + num(S ? S->src_pad : -1) + " (";
    for (long long v : args) s += " " + num(v);
    const bool no = decline && !where.empty() && (!std::strcmp(decline, "*") || !std::strcmp(decline, name));
    line(s + " ) on " + stream(q) + (no ? " -> declines" : ""));
    return no ? 1 : 0;
}
int launch(const char *name, const PcState *S, std::initializer_list<long long> args, hipStream_t q) { return launch(name, "", S, args, q); }
// ... for R runs: where their records are in the uploaded block
int launch_many(const char *name, const PcState *S, const PcManyRec *d, int R, std::initializer_list<long long> args, hipStream_t q)
{
    return launch(name, " records " + num(d - dev_block) + "+" + num(R), S, args, q);
}
long long P(const void *p) { return (long long)(uintptr_t)p; }
}

#define HIPCHK(x) (void)(x)
#define hipEventRecord(e, q) rec::event_record(e, q)
#define hipStreamWaitEvent(q, e, flags) rec::stream_wait(q, e)
#define hipEventSynchronize(e) rec::event_sync(e)
#define hipMemcpyAsync(dst, src, bytes, kind, q) rec::upload(dst, src, bytes, q)

template <class T> T *halloc(size_t n) { rec::line("host block of " + rec::num((long long)n)); return (T *)std::calloc(n, sizeof(T)); }
void hfree(void *p) { rec::line("host block freed"); std::free(p); }
template <class T> T *dalloc(size_t n) { rec::line("device block of " + rec::num((long long)n)); return (T *)std::calloc(n, sizeof(T)); }
template <class T> void dfree(T *&p) { rec::line("device block freed"); std::free((void *)p); p = nullptr; }
struct EventPool {
    uintptr_t next = 0x1000;
    hipEvent_t get_sync_event() { rec::line("event taken"); return (hipEvent_t)(next += 16); }
    void put_sync_event(hipEvent_t) { rec::line("event given back"); }
};
EventPool &hpool() { static EventPool p; return p; }
static void pc_copy_many(const std::vector<std::array<uintptr_t, 3>> &reqs, hipStream_t q)
{
    std::string s = "copies on " + rec::stream(q) + ":";
    for (const auto &c : reqs) s += " " + rec::num((long long)c[0]) + "<-" + rec::num((long long)c[1]) + "x" + rec::num((long long)c[2]);
    rec::line(s);
}

#ifdef COHORT_PARENT
#include COHORT_PARENT
#else
#include "pc_cohort.h"
#endif

std::string rec::stream(hipStream_t q) { return q == cur->st ? "main" : (q == cur->st2 && q) ? "second" : "?"; }
std::string rec::event(hipEvent_t e)
{
    if (e && e == cur->ev_up) return "upload";
    if (e && e == cur->ev_next) return "next";
    for (int k = 0; k < 4; ++k) if (e && e == cur->ev_seq[k]) return "ev_seq[" + num(k) + "]";
    for (int k = 0; k < Cohort::RING; ++k) { if (e && e == cur->ev[k]) return "slot[" + num(k) + "]"; if (e && e == cur->ev2[k]) return "slot2[" + num(k) + "]"; }
    return "?";
}

// ---- the launchers
using rec::P;
extern "C" {
void pc_launch_clean(const PcState *S, int nph, unsigned char *keep, int *blk, int *d_total, double *ph2, double *phL2, unsigned *phC2, unsigned long long *phU2, int *dst_index, hipStream_t st)
{ rec::launch("clean", S, {nph, P(keep), P(blk), P(d_total), P(ph2), P(phL2), P(phC2), P(phU2), P(dst_index)}, st); }
int pc_launch_clean_many(const PcManyRec *dR, int R, int nblk_max, hipStream_t st) { return rec::launch_many("clean_many", nullptr, dR, R, {nblk_max}, st); }
void pc_launch_reset_thresholds(const PcState *S, hipStream_t st) { rec::launch("reset_thresholds", S, {}, st); }
int pc_launch_reset_thresholds_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st) { return rec::launch_many("reset_thresholds_many", S, dR, R, {}, st); }
int pc_launch_knn_cluster_batch_dev(const PcState *S, const int *d_desc, int nd, int nmax, double *Sm, int *knn, int *labels, int *out, const int *dims, int ndims, hipStream_t st)
{ return rec::launch("knn_cluster_batch_dev", S, {P(d_desc), nd, nmax, P(Sm), P(knn), P(labels), P(out), P(dims), ndims}, st); }
int pc_launch_knn_cluster_batch_many(const PcState *S, const PcManyRec *dR, int R, int nd_max, int nmax, int any_sub, hipStream_t st)
{ return rec::launch_many("knn_cluster_batch_many", S, dR, R, {nd_max, nmax, any_sub}, st); }
int pc_launch_knn_cluster_sub(const int *d_desc, int nb, int mmax, const double *Sm, const int *pool, int *knn, int *labels, int *out, hipStream_t st)
{ return rec::launch("knn_cluster_sub", nullptr, {P(d_desc), nb, mmax, P(Sm), P(pool), P(knn), P(labels), P(out)}, st); }
int pc_launch_knn_cluster_sub_many(const PcManyRec *dR, int R, int nb_max, int mmax, hipStream_t st) { return rec::launch_many("knn_cluster_sub_many", nullptr, dR, R, {nb_max, mmax}, st); }
int pc_launch_nhats_part(const PcState *S, unsigned batch, int nchains, int part, hipStream_t st, int packed) { return rec::launch("nhats_part", S, {batch, nchains, part, packed}, st); }
int pc_launch_bases_t_many(const PcState *S, const PcManyRec *dR, int R, unsigned batch, int nchains, hipStream_t st) { return rec::launch_many("bases_t_many", S, dR, R, {batch, nchains}, st); }
int pc_launch_nhats(const PcState *S, unsigned batch, int nchains, hipStream_t st) { return rec::launch("nhats", S, {batch, nchains}, st); }
int pc_launch_nhats_many(const PcState *S, const PcManyRec *dR, int R, int nchains, hipStream_t st) { return rec::launch_many("nhats_many", S, dR, R, {nchains}, st); }
int pc_launch_slice_t(const PcState *S, unsigned batch, int nchains, hipStream_t st) { return rec::launch("slice_t", S, {batch, nchains}, st); }
int pc_launch_slice_t_many(const PcState *S, const PcManyRec *dR, int R, unsigned batch, int nchains, hipStream_t st) { return rec::launch_many("slice_t_many", S, dR, R, {batch, nchains}, st); }
int pc_launch_slice(const PcState *S, unsigned batch, int nchains, hipStream_t st) { return rec::launch("slice", S, {batch, nchains}, st); }
int pc_launch_slice_fused(const PcState *S, unsigned batch, int nchains, hipStream_t st) { return rec::launch("slice_fused", S, {batch, nchains}, st); }
int pc_launch_slice_many(const PcState *S, const PcManyRec *dR, int R, int nchains, int fused, hipStream_t st) { return rec::launch_many("slice_many", S, dR, R, {nchains, fused}, st); }
int pc_launch_slice_step(const PcState *S, const PcManyRec *dR, int R, int nchains, int fused, hipStream_t st) { return rec::launch_many("slice_step", S, dR, R, {nchains, fused}, st); }
// (the tick stage of the device batch callback, CK_TICK: named by the table, in no scenario here -- the parent has no such stage)
void pc_launch_slice_tick_dev(const PcState *S, unsigned batch, int nchains, void *, double *, int *, double *, const double *, const double *, const double *, int first, const int *, hipStream_t st) { rec::launch("slice_tick_dev", S, {batch, nchains, first}, st); }
int pc_launch_slice_tick_many(const PcManyRec *dR, int R, int nchains, hipStream_t st) { return rec::launch_many("slice_tick_many", nullptr, dR, R, {nchains}, st); }
int pc_launch_sort_live(const PcState *S, hipStream_t st) { return rec::launch("sort_live", S, {}, st); }
int pc_launch_sort_live_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st) { return rec::launch_many("sort_live_many", S, dR, R, {}, st); }
void pc_launch_nn_lists(const PcState *S, int nleft, int use_rank, hipStream_t st) { rec::launch("nn_lists", S, {nleft, use_rank}, st); }
int pc_launch_nn_lists_many(const PcState *S, const PcManyRec *dR, int R, int nleft_max, int use_rank, hipStream_t st) { return rec::launch_many("nn_lists_many", S, dR, R, {nleft_max, use_rank}, st); }
int pc_launch_consume_par(const PcState *S, hipStream_t st) { return rec::launch("consume_par", S, {}, st); }
int pc_launch_consume_par_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st) { return rec::launch_many("consume_par_many", S, dR, R, {}, st); }
int pc_launch_consume_cl(const PcState *S, int nc, hipStream_t st) { return rec::launch("consume_cl", S, {nc}, st); }
int pc_launch_consume_cl_many(const PcState *S, const PcManyRec *dR, int R, int wide, hipStream_t st) { return rec::launch_many("consume_cl_many", S, dR, R, {wide}, st); }
void pc_launch_apply(const PcState *S, unsigned batch, int nchains, hipStream_t st) { rec::launch("apply", S, {batch, nchains}, st); }
int pc_launch_apply_many(const PcState *S, const PcManyRec *dR, int R, unsigned batch, int nchains, hipStream_t st) { return rec::launch_many("apply_many", S, dR, R, {batch, nchains}, st); }
void pc_launch_update_fused(const PcState *S, int nph, unsigned char *keep, int *blk, int *d_total, double *ph2, double *phL2, unsigned *phC2, unsigned long long *phU2, double *part, double *shift, int deferred, hipStream_t st)
{ rec::launch("update_fused", S, {nph, P(keep), P(blk), P(d_total), P(ph2), P(phL2), P(phC2), P(phU2), P(part), P(shift), deferred}, st); }
int pc_launch_update_fused_many(const PcState *S, const PcManyRec *dR, int R, int nblk_max, int G, int deferred, hipStream_t st) { return rec::launch_many("update_fused_many", S, dR, R, {nblk_max, G, deferred}, st); }
int pc_launch_final_par(const PcState *S, hipStream_t st) { return rec::launch("final_par", S, {}, st); }
int pc_launch_final_par_many(const PcManyRec *dR, int R, hipStream_t st) { return rec::launch_many("final_par_many", nullptr, dR, R, {}, st); }
}

// ---- a record's arguments, drawn before it is written down (the same draws whichever Cohort is driven), and the two ways to write it down
struct Args {
    void *p[9];               // buffers (fabricated addresses, all different)
    unsigned batch; int nchains, nph, grid, deferred, nd, nmax, nd_sub, nb, mmax, nleft, fused, wide, bases_seq;
};
template <class T> static T *as(void *p) { return (T *)p; }
static void write_down(Cohort &c, int kind, const PcState &S, const Args &a)
{
#ifdef COHORT_PARENT
    // (the brace lists of abd2406's call sites, pc_engine.hip:1200 .. 2610)
    void *const *p = a.p;
    switch (kind) {
    case CK_COMPACT: c.rec(CK_COMPACT, S, {p[0], p[1], p[2], p[3], p[4], p[5], p[6]}, {}, {0, a.nph, (a.nph + 255) / 256}); break;
    case CK_UPDATE: c.rec(CK_UPDATE, S, {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}, {(long long)a.grid, a.deferred ? 1LL : 0LL}, {0, a.nph, (a.nph + 255) / 256}); break;
    case CK_RESET: c.rec(CK_RESET, S, {}, {}, {}); break;
    case CK_CLUSG: c.rec(CK_CLUSG, S, {p[0], p[1], p[2], p[3], p[4], p[5]}, {}, {0, a.nb, a.mmax}); break;
    case CK_CLUS1: c.rec(CK_CLUS1, S, {p[0], p[1], p[2], p[3], p[4], p[5]}, {}, {0, a.nd, a.nmax, a.nd_sub}); break;
    case CK_BASES: c.rec(CK_BASES, S, {}, {(long long)a.nchains}, {(int)a.batch}); break;
    case CK_NHATS_G: c.rec(CK_NHATS_G, S, {}, {(long long)a.nchains}, {(int)a.batch}); break;
    case CK_SLICE: c.rec(CK_SLICE, S, {}, {(long long)a.nchains}, {(int)a.batch, 0, 0, a.bases_seq}); break;
    case CK_SLICE_G: c.rec(CK_SLICE_G, S, {}, {(long long)a.nchains, a.fused ? 1LL : 0LL}, {(int)a.batch, 0, 0, a.fused ? a.bases_seq : 0}); break;
    case CK_BASES_NEXT: c.rec(CK_BASES_NEXT, S, {}, {(long long)a.nchains}, {(int)a.batch}); break;
    case CK_SORT: c.rec(CK_SORT, S, {}, {}, {}); break;
    case CK_NN: c.rec(CK_NN, S, {}, {}, {0, a.nleft}); break;
    case CK_CONSUME: c.rec(CK_CONSUME, S, {}, {}, {}); break;
    case CK_CONSUME_CL: c.rec(CK_CONSUME_CL, S, {}, {a.wide ? 1LL : 0LL}, {}); break;
    case CK_APPLY: c.rec(CK_APPLY, S, {}, {(long long)a.nchains}, {(int)a.batch}); break;
    case CK_FINAL: c.rec(CK_FINAL, S, {}, {}, {}); break;
    }
#else
    void *const *p = a.p;
    if (kind == CK_COMPACT) c.rec(rec_compact(S, as<unsigned char>(p[0]), as<int>(p[1]), as<int>(p[2]), as<double>(p[3]), as<double>(p[4]), as<unsigned>(p[5]), as<unsigned long long>(p[6]), a.nph));
    else if (kind == CK_UPDATE) c.rec(rec_update(S, as<unsigned char>(p[0]), as<int>(p[1]), as<int>(p[2]), as<double>(p[3]), as<double>(p[4]), as<unsigned>(p[5]), as<unsigned long long>(p[6]),
                                                  as<double>(p[7]), as<double>(p[8]), a.grid, a.deferred != 0, a.nph));
    else if (kind == CK_RESET) c.rec(rec_reset(S));
    else if (kind == CK_CLUSG) c.rec(rec_clusg(S, as<int>(p[0]), as<double>(p[1]), as<int>(p[2]), as<int>(p[3]), as<int>(p[4]), as<int>(p[5]), a.nb, a.mmax));
    else if (kind == CK_CLUS1) c.rec(rec_clus1(S, as<int>(p[0]), as<double>(p[1]), as<int>(p[2]), as<int>(p[3]), as<int>(p[4]), as<const int>(p[5]), a.nd, a.nmax, a.nd_sub));
    else if (kind == CK_BASES) c.rec(rec_bases(S, a.batch, a.nchains));
    else if (kind == CK_NHATS_G) c.rec(rec_nhats_g(S, a.batch, a.nchains));
    else if (kind == CK_SLICE) c.rec(rec_slice(S, a.batch, a.nchains, a.bases_seq));
    else if (kind == CK_SLICE_G) c.rec(rec_slice_g(S, a.batch, a.nchains, a.fused != 0, a.fused ? a.bases_seq : 0));
    else if (kind == CK_BASES_NEXT) c.rec(rec_bases_next(S, a.batch, a.nchains));
    else if (kind == CK_SORT) c.rec(rec_sort(S));
    else if (kind == CK_NN) c.rec(rec_nn(S, a.nleft));
    else if (kind == CK_CONSUME) c.rec(rec_consume(S));
    else if (kind == CK_CONSUME_CL) c.rec(rec_consume_cl(S, a.wide != 0));
    else if (kind == CK_APPLY) c.rec(rec_apply(S, a.batch, a.nchains));
    else if (kind == CK_FINAL) c.rec(rec_final(S));
#endif
}

static const int KINDS[] = { CK_COMPACT, CK_RESET, CK_CLUS1, CK_CLUSG, CK_BASES, CK_NHATS_G, CK_SLICE, CK_SLICE_G, CK_BASES_NEXT, CK_SORT, CK_NN, CK_CONSUME, CK_CONSUME_CL, CK_APPLY, CK_UPDATE, CK_FINAL };
static const char *const KIND_NAMES[] = { "compact", "reset", "clus1", "clusg", "bases", "nhats_g", "slice", "slice_g", "bases_next", "sort", "nn", "consume", "consume_cl", "apply", "update", "final" };
static const char *const MANY_OF[] = { "clean_many", "reset_thresholds_many", "knn_cluster_batch_many", "knn_cluster_sub_many", "bases_t_many", "nhats_many", "slice_t_many", "slice_many",
                                       "bases_t_many", "sort_live_many", "nn_lists_many", "consume_par_many", "consume_cl_many", "apply_many", "update_fused_many", "final_par_many" };
static constexpr int NK = sizeof(KINDS) / sizeof(KINDS[0]);

struct Gen {
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    unsigned next(unsigned m) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((s >> 33) % m); }
};
static Gen gen;
static PcState state_of(int run)
{
    PcState S;
    std::memset(&S, 0, sizeof S);
    S.src_pad = run; S.D = 8; S.nr = 16; S.N = 100; S.Ncap = 128; S.B = 32; S.pool = 1;
    return S;
}
// the shared words the same for every run (a launch's runs must agree on them), each run's own integers and buffers drawn
static Args args_of(int run)
{
    Args a;
    for (int i = 0; i < 9; ++i) a.p[i] = (void *)(uintptr_t)(0x100000u * (unsigned)(run + 1) + 0x100u * (unsigned)(i + 1));
    a.batch = 7; a.nchains = 32; a.grid = 12; a.deferred = 0; a.fused = 1; a.wide = 0;
    a.nph = 1 + (int)gen.next(5000); a.nd = 1 + (int)gen.next(9); a.nmax = 3 + (int)gen.next(200); a.nd_sub = (int)gen.next(3) == 0 ? 2 : 0;
    a.nb = 1 + (int)gen.next(20); a.mmax = 3 + (int)gen.next(100); a.nleft = 2 + (int)gen.next(30); a.bases_seq = 0;
    return a;
}
static void init(Cohort &c, bool second)
{
    rec::cur = &c;
    c.st = (hipStream_t)(uintptr_t)0x10;
    if (second) { c.st2 = (hipStream_t)(uintptr_t)0x20; c.ev_up = (hipEvent_t)(uintptr_t)0x30; c.ev_next = (hipEvent_t)(uintptr_t)0x40; }
}
static void state(const Cohort &c)
{
    rec::line("fused " + rec::num(c.n_fused) + " single " + rec::num(c.n_single) + " launched " + rec::num((long long)c.seq_launched) + " waited " + rec::num((long long)c.seq_waited) +
              " next_pending " + rec::num(c.next_pending) + " cap " + rec::num((long long)c.cap) + " pending " + rec::num((long long)c.pend.size()));
}
static void flush(Cohort &c) { rec::line("-- flush"); c.flush(); state(c); }

static bool dump = false;
static void scenario(const std::string &name, const std::function<void()> &body)
{
    rec::text.clear(); rec::decline = nullptr;
    body();
    unsigned long long h = 1469598103934665603ull; long lines = 0;
    for (unsigned char ch : rec::text) { h ^= ch; h *= 1099511628211ull; lines += ch == '\n'; }
    std::printf("%s %016llx %ld\n", name.c_str(), h, lines);
    if (dump) std::printf("%s", rec::text.c_str());
}

int main(int argc, char **argv)
{
    dump = argc > 1 && !std::strcmp(argv[1], "--dump");
    // every kind, in groups of 1, 2, 5 and 64 runs, the second stream there and not
    for (int second = 0; second < 2; ++second)
        for (int k = 0; k < NK; ++k)
            scenario(std::string("group_") + KIND_NAMES[k] + (second ? "_st2" : ""), [&] {
                Cohort c; init(c, second != 0);
                for (int n : {1, 2, 5, 64}) { for (int r = 0; r < n; ++r) write_down(c, KINDS[k], state_of(r), args_of(r)); flush(c); }
                c.destroy();
            });
    // runs that differ in each key of the order in turn, two of each, written down in a drawn order (the sort is stable)
    for (int k = 0; k < NK; ++k)
        scenario(std::string("keys_") + KIND_NAMES[k], [&] {
            Cohort c; init(c, true);
            static double lo[1];
            for (int pass = 0; pass < 3; ++pass) {
                std::vector<int> order;
                for (int v = 0; v < 10; ++v) { order.push_back(v); order.push_back(v); }
                for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[gen.next((unsigned)i)]);
                for (size_t r = 0; r < order.size(); ++r) {
                    PcState S = state_of((int)r); Args a = args_of((int)r);
                    switch (order[r]) {
                    case 1: S.Ncap = 256; break;
                    case 2: S.B = 64; break;
                    case 3: S.pool = 0; break;
                    case 4: S.prior.lo = lo; break;
                    case 5: a.nchains = 64; break;                 // the words of Rec::a, where the kind has them
                    case 6: a.fused = 0; break;
                    case 7: a.grid = 20; break;
                    case 8: a.deferred = 1; break;
                    case 9: a.wide = 1; break;
                    }
                    write_down(c, KINDS[k], S, a);
                }
                flush(c);
            }
            c.destroy();
        });
    // each _many launcher declines, the one of the other kind in the same flush does not: the one-run launches are taken for the one
    for (int second = 0; second < 2; ++second)
        for (int k = 0; k < NK; ++k)
            scenario(std::string("declines_") + KIND_NAMES[k] + (second ? "_st2" : ""), [&] {
                Cohort c; init(c, second != 0);
                rec::decline = MANY_OF[k];
                for (int r = 0; r < 3; ++r) { Args a = args_of(r); a.fused = r & 1; a.wide = r == 2; a.deferred = r & 1; write_down(c, KINDS[k], state_of(r), a); }
                for (int r = 3; r < 5; ++r) write_down(c, KINDS[(k + 1) % NK], state_of(r), args_of(r));
                flush(c);
                c.destroy();
            });
    // whole rounds of sixteen runs, every kind drawn, more flushes in a row than the ring has slots, a flush that outgrows the block
    for (int second = 0; second < 2; ++second)
        for (int all_decline = 0; all_decline < 2; ++all_decline)
            scenario(std::string("rounds") + (second ? "_st2" : "") + (all_decline ? "_declined" : ""), [&] {
                Cohort c; init(c, second != 0);
                if (all_decline) rec::decline = "*";
                for (int round = 0; round < 12; ++round) {
                    const int nruns = round < 3 ? 3 : round == 8 ? 40 : 16;      // (cap: 6 records a run's worth, then outgrown twice)
                    for (int r = 0; r < nruns; ++r) {
                        const int nrec = 1 + (int)gen.next(4);
                        for (int q = 0; q < nrec; ++q) {
                            Args a = args_of(r); PcState S = state_of(r);
                            a.batch = (unsigned)round; a.fused = (int)gen.next(2); a.wide = (int)gen.next(4) == 0; a.deferred = (int)gen.next(2); a.grid = 8 + 4 * (int)gen.next(2);
                            a.bases_seq = (int)gen.next((unsigned)c.seq_launched + 3);
                            if (gen.next(5) == 0) S.Ncap = 256;
                            write_down(c, KINDS[gen.next(NK)], S, a);
                        }
                    }
                    flush(c);
                }
                c.destroy();
            });
    // the numbered wait for the bases: 0 (drawn in line), launched and not waited for, waited for, not yet launched; a group that mixes them
    for (int second = 0; second < 2; ++second)
        for (int kind : {CK_SLICE, CK_SLICE_G})
            scenario(std::string("bases_number_") + (kind == CK_SLICE ? "slice" : "slice_g") + (second ? "_st2" : ""), [&] {
                Cohort c; init(c, second != 0);
                auto slices = [&](std::initializer_list<int> seqs) { int r = 0; for (int s : seqs) { Args a = args_of(r); a.bases_seq = s; write_down(c, kind, state_of(r), a); ++r; } };
                auto bases = [&](int n) { for (int r = 0; r < n; ++r) { Args a = args_of(r); a.batch = 8; write_down(c, CK_BASES_NEXT, state_of(r), a); } };
                slices({0, 0}); flush(c);                                  // in line, nothing pending
                bases(2); flush(c);                                        // launch 1
                slices({0}); flush(c);                                     // in line, the second stream's latest pending
                bases(2); slices({1, 1}); flush(c);                        // launched (1), not waited for; launch 2 behind it in the same flush
                slices({1, 1}); flush(c);                                  // waited for
                slices({2, 1}); flush(c);                                  // the later of the two
                slices({3, 3}); flush(c);                                  // not yet launched
                bases(1); flush(c); bases(1); flush(c); bases(1); flush(c); bases(1); flush(c);      // launches 3 .. 6: the four events go round
                slices({2, 0}); flush(c);                                  // one of the group in line: not numbered
                slices({6, 5, 4}); flush(c);
                slices({7}); bases(3); flush(c);                           // its bases in the same flush, behind it
                slices({7}); flush(c);
                c.destroy();
            });
    // nothing written down: the copies and closures asked for in front and behind
    for (int second = 0; second < 2; ++second)
        scenario(std::string("empty_flush") + (second ? "_st2" : ""), [&] {
            Cohort c; init(c, second != 0);
            c.pre.push_back([] { rec::line("closure in front 1"); }); c.pre.push_back([] { rec::line("closure in front 2"); });
            c.post.push_back([] { rec::line("closure behind 1"); }); c.post.push_back([] { rec::line("closure behind 2"); });
            c.pre_copies.push_back({1, 2, 3}); c.post_copies.push_back({4, 5, 6}); c.post_copies.push_back({7, 8, 9});
            flush(c);
            flush(c);                                                      // (and nothing at all)
            c.post.push_back([&c] { rec::line("closure behind that asks for another"); c.post.push_back([] { rec::line("the other"); }); });
            write_down(c, CK_APPLY, state_of(0), args_of(0));
            c.pre_copies.push_back({10, 11, 12});
            flush(c); flush(c);
            c.destroy();
        });
    return 0;
}
