// split_record.hip -- what the host's half of a clustering update (pc_split.h: ClusterUpdate and the pure steps above it) sends to the device,
// launches or writes down for the runs in step, fetches and waits for, recorded on the CPU.
//
// Includes pc_split.h with a scripted stand-in for Engine (the members the header's head comment lists, and no others), a scripted device and
// recorders for the launchers and the cohort's records.  Device blocks are host memory; a record names an address by the block's role and the
// offset in it.  The scripted device answers a clustering launch with labels that depend on the part's point set only (the premise of the
// level-by-level recursion): every live slot carries a path of digits, a set of points splits by the first digit its paths do not share, and
// is one cluster when they share all.  No device, no kernel runs.  Built host-only (make -C polychordlite_amd/csrc split_record);
// tests/test_split_record.py compares the digests with those of the code before the header (9f0f34b).
//
//   split_record              one line per scenario: its name, the digest of its record, the number of lines
//   split_record --dump       the records themselves
//   split_record --order      (not with SPLIT_PARENT) PartRefiner against the reference's depth-first order (clustering.f90:80-95, restated
//                             below with relabel by first appearance, utils.F90:713-749) over seeded random clusters of 3 ... 200 points, the
//                             rule "split by a hash of the smallest index until a part is at most k points": final labels and counts must be
//                             identical; prints the clusters tried and the mismatches
//   split_record --split      (not with SPLIT_PARENT) the two pure steps of add_cluster on a fabricated 4-cluster state: inputs and outputs as
//                             hexadecimal doubles, for the test to hold against the oracle's formulas
// With -DSPLIT_PARENT='"FILE"' (make split_record_parent SPLIT_PARENT='"FILE"': its own binary, split_record_parent) the same scenarios drive
// FILE instead, included inside the scripted Engine: lines 1292-1604 of 9f0f34b's pc_engine.hip behind four lines that stand in for what that text names
// and this tree no longer has (the recipe is in CHANGELOG.md, the entry of pc_split.h, and only there: it has to spell the removed names).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <cstdarg>
#include <cmath>
#include <string>
#include <vector>
#include <map>
#include <atomic>
#include <functional>
#include <algorithm>
#include "polychord_hip.h"
#include "pc_state.h"
#include "pc_launch.h"

enum { PC_RC_DEVICE = 2, PC_RC_LDS = 4, PC_RC_MEMORY = 7, PC_RC_LIMIT = 8 };      // (the record shows a failure's code as the scenario gives it)
struct EngineError { int code; std::string msg; };
[[noreturn]] static void engine_fail(int code, const char *fmt, ...)
{
    char buf[512]; va_list ap; va_start(ap, fmt); std::vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    throw EngineError{code, buf};
}
static std::atomic<int> g_inject_fault{0};
#define HIPCHK(x) (void)(x)
#define hipMemcpyAsync(dst, src, bytes, kind, q) hipSuccess

static unsigned long long fnv(const void *p, size_t n, unsigned long long h = 1469598103934665603ull)
{
    for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char *)p)[i]; h *= 1099511628211ull; }
    return h;
}
static unsigned mix(unsigned a, unsigned b) { unsigned long long h = fnv(&a, 4); h = fnv(&b, 4, h); return (unsigned)(h ^ (h >> 32)); }

struct Engine;
namespace rec {
std::string text;
Engine *eng = nullptr;
void line(const std::string &s) { text += s; text += '\n'; }
std::string num(long long v) { return std::to_string(v); }
std::string hex(unsigned long long v) { char b[24]; std::snprintf(b, sizeof b, "%016llx", v); return b; }
std::map<const char *, size_t> blocks;              // the device blocks there are: base -> bytes
std::string tag(const void *p);                     // role + offset (behind Engine)
}

template <class T> T *dalloc(size_t n) { T *p = (T *)std::calloc(n ? n : 1, sizeof(T)); rec::blocks[(const char *)p] = (n ? n : 1) * sizeof(T); return p; }
template <class T> void dfree(T *&p) { if (p) { rec::blocks.erase((const char *)p); std::free((void *)p); } p = nullptr; }
// (the run's ledger over these: the clustering scratch is allocated through it; an update takes no pinned block)
void dfree(const std::vector<void *> &ps) { for (void *p : ps) dfree(p); }
template <class T> T *halloc(size_t n) { return (T *)std::calloc(n ? n : 1, sizeof(T)); }
void hfree(void *p) { std::free(p); }
#define PC_BLOCKS_OWN_PRIMITIVES
#include "pc_blocks.h"

// ---- the cohort of the runs in step, as far as an update sees it: records written down, launched at the next flush
struct Cohort {
    struct Rec { std::string what; std::function<void()> run; };
    std::vector<Rec> pend;
    void rec(const Rec &r) { rec::line("written down: " + r.what); pend.push_back(r); }
    void flush()
    {
        rec::line("flush: " + rec::num((long long)pend.size()) + " records");
        std::vector<Rec> p; p.swap(pend);
        for (Rec &r : p) r.run();
    }
};

static Cohort::Rec rec_clus1(const PcState &S, int *desc, double *Sm, int *knn, int *lab, int *out, const int *dims, int nd, int nmax, int nd_sub);
static Cohort::Rec rec_clusg(const PcState &S, int *desc, double *Sm, int *pool, int *knn, int *lab, int *out, int nb, int mmax);

// ---- the scripted device
namespace devs {
const int PATH = 6;
std::map<int, std::vector<int>> path[2];            // slot -> digits: [0] the full pass, [1] the sub-dimension pass
std::vector<int> last_desc; int last_sub = 0;        // the first pass' descriptors, and whether it was a sub-dimension pass
// one pass of NN_clustering over a set of slots: labels 1 .. num by first appearance
int cluster_once(const std::vector<int> &slots, int sub, std::vector<int> &lab)
{
    const int m = (int)slots.size();
    lab.assign((size_t)m, 1);
    int at = 0;
    for (; at < PATH; ++at) { bool same = true; for (int s : slots) same = same && path[sub].at(s)[(size_t)at] == path[sub].at(slots[0])[(size_t)at]; if (!same) break; }
    if (at == PATH) return 1;
    std::vector<int> seen;
    for (int a = 0; a < m; ++a) {
        const int d = path[sub].at(slots[(size_t)a])[(size_t)at];
        size_t f = std::find(seen.begin(), seen.end(), d) - seen.begin();
        if (f == seen.size()) seen.push_back(d);
        lab[(size_t)a] = (int)f + 1;
    }
    return (int)seen.size();
}
void first_pass(const PcState *S, const int *desc, int nd, int *labels, int *out, int sub)
{
    last_desc.assign(desc, desc + 4 * nd); last_sub = sub;
    for (int k = 0; k < nd; ++k) {
        const int c = desc[4 * k], n = desc[4 * k + 1], o1 = desc[4 * k + 3];
        std::vector<int> slots(S->cl_list + (size_t)c * S->Ncap, S->cl_list + (size_t)c * S->Ncap + n), lab;
        out[k] = cluster_once(slots, sub, lab);
        std::copy(lab.begin(), lab.end(), labels + o1);
    }
}
void level(const PcState *S, const int *g, int nb, const int *pool, int *labels, int *out)
{
    for (int b = 0; b < nb; ++b, g += 5) {
        int c = -1;
        for (size_t k = 0; 4 * k < last_desc.size(); ++k) if (last_desc[4 * k + 2] == g[0] && last_desc[4 * k + 1] == g[1]) c = last_desc[4 * k];
        std::vector<int> slots, lab;
        for (int a = 0; a < g[3]; ++a) slots.push_back(S->cl_list[(size_t)c * S->Ncap + pool[g[2] + a]]);
        out[b] = cluster_once(slots, last_sub, lab);
        std::copy(lab.begin(), lab.end(), labels + g[2]);
    }
}
void rebuild(const PcState *S, int nc)
{
    for (int c = 0; c < nc; ++c) S->cl_n[c] = 0;
    for (int s = 0; s < S->Ncap; ++s) { const int c = S->live_cluster[s]; if (c < 0 || c >= nc) continue; S->cl_list[(size_t)c * S->Ncap + S->live_pos[s]] = s; S->cl_n[c]++; }
}
void ph_rehome(const PcState *S, int nph, int nc, int *counts) { for (int c = 0; c < nc; ++c) counts[c] = (int)(mix(S->cl_uid[c], (unsigned)nph) % 50u); }
}

// ---- the scripted engine
#ifndef SPLIT_PARENT
#include "pc_split.h"
#endif
struct Settings { int epoch_discard = 0; };
struct Engine {
    Cohort *co = nullptr;
    Settings cfg;
    RunBlocks blocks;
    PcState S{}; PcCtl *h_ctl = nullptr; hipStream_t st = (hipStream_t)(uintptr_t)0x1000;
    long nsplits = 0; int ncluster_peak = 1;
    std::vector<unsigned> split_child, split_parent; std::vector<double> split_logfrac;
    struct Fetch { void *dst; const void *src; size_t bytes; };
    std::vector<Fetch> fetching;
    void direct_op() { if (co) co->flush(); }
    void fetch_raw(void *dst, const void *src, size_t bytes)
    {
        if (!bytes) return;
        rec::line("fetch " + rec::tag(src) + " " + rec::num((long long)bytes) + " bytes");
        fetching.push_back({dst, src, bytes});
    }
    template <class T> void fetch(std::vector<T> &v, const T *p, size_t n) { v.resize(n); fetch_raw(v.data(), p, sizeof(T) * n); }
    void fetch_wait()
    {
        if (co) co->flush();
        rec::line("wait");
        for (const Fetch &f : fetching) std::memcpy(f.dst, f.src, f.bytes);
        fetching.clear();
    }
    void send(const char *how, void *dst, const void *src, size_t bytes)
    {
        rec::line(std::string(how) + " " + rec::tag(dst) + " " + rec::num((long long)bytes) + " bytes " + rec::hex(fnv(src, bytes)));
        std::memcpy(dst, src, bytes);
    }
    void send_raw(void *dst, const void *src, size_t bytes) { if (!bytes) return; direct_op(); send("send", dst, src, bytes); }
    void send_pre(void *dst, const void *src, size_t bytes) { if (!bytes) return; if (!co) { send_raw(dst, src, bytes); return; } send("send ahead", dst, src, bytes); }
    // (as Engine::grow_clusters: the stream drained, every per-cluster array with room for twice as many, the matrix with its new leading dimension)
    void grow_clusters(int need)
    {
        const int mo = S.maxc, mn = std::max(need, 2 * mo);
        rec::line("the list of clusters grows from " + rec::num(mo) + " to " + rec::num(mn));
        if (co) co->flush();
        rec::line("host waits for the stream");
        auto grow = [&](auto *&p, size_t no, size_t nn) { auto *q = dalloc<typename std::remove_reference<decltype(*p)>::type>(nn); std::memcpy(q, p, sizeof(*p) * no); dfree(p); p = q; };
        grow(S.logXp, mo, mn); grow(S.logZXp, mo, mn); grow(S.logZp, mo, mn); grow(S.logZp2, mo, mn); grow(S.logZpXp, mo, mn); grow(S.death_thr, mo, mn);
        grow(S.cl_n, mo, mn); grow(S.cl_uid, mo, mn); grow(S.cl_list, (size_t)mo * S.Ncap, (size_t)mn * S.Ncap);
        {
            double *q = dalloc<double>(2 * (size_t)mn * mn);
            for (int a = 0; a < mo; ++a) std::copy(S.XpXq + (size_t)a * mo, S.XpXq + (size_t)(a + 1) * mo, q + (size_t)a * mn);
            dfree(S.XpXq); S.XpXq = q;
        }
#ifdef SPLIT_PARENT
        if (c_cnt) { dfree(c_cnt); dfree(c_olduid); c_cnt = dalloc<int>(mn); c_olduid = dalloc<unsigned>(mn); }
#else
        clus.regrow_counts(mn);
#endif
        S.maxc = mn;
    }
#ifdef SPLIT_PARENT
    double *c_Sm = nullptr; int *c_pts = nullptr, *c_gidx = nullptr, *c_knn = nullptr, *c_lab = nullptr, *c_out = nullptr, *c_cnt = nullptr;
    unsigned *c_olduid = nullptr; int c_cap = 0;
#include SPLIT_PARENT
#define CLUS(e) (e)
#else
    ClusterUpdate<Engine> clus{*this};
    std::vector<int> sub_dims; int *c_subdims = nullptr;
#define CLUS(e) ((e).clus)
#endif
};

std::string rec::tag(const void *p)
{
    if (!p) return "null";
    Engine &e = *eng;
    const std::pair<const void *, const char *> roles[] = {
        {e.S.live_cluster, "live_cluster"}, {e.S.live_pos, "live_pos"}, {e.S.logXp, "logXp"}, {e.S.logZXp, "logZXp"}, {e.S.logZp, "logZp"}, {e.S.logZp2, "logZp2"},
        {e.S.logZpXp, "logZpXp"}, {e.S.death_thr, "death_thr"}, {e.S.XpXq, "XpXq"}, {e.S.cl_uid, "cl_uid"}, {e.S.cl_n, "cl_n"}, {e.S.cl_list, "cl_list"}, {e.S.ctl, "ctl"},
        {e.c_subdims, "c_subdims"}, {CLUS(e).c_Sm, "c_Sm"}, {CLUS(e).c_knn, "c_knn"}, {CLUS(e).c_lab, "c_lab"}, {CLUS(e).c_cnt, "c_cnt"}, {CLUS(e).c_olduid, "c_olduid"},
        {CLUS(e).c_desc, "c_desc"}, {CLUS(e).c_bout, "c_bout"}, {CLUS(e).c_gdesc, "c_gdesc"}, {CLUS(e).c_gpool, "c_gpool"}, {CLUS(e).c_glab, "c_glab"},
        {CLUS(e).c_gout, "c_gout"}, {CLUS(e).c_map, "c_map"}};
    for (auto &r : roles) {
        auto it = r.first ? blocks.find((const char *)r.first) : blocks.end();
        if (it != blocks.end() && (const char *)p >= it->first && (const char *)p < it->first + it->second) return std::string(r.second) + "+" + num((const char *)p - it->first);
    }
    return "an address outside every block";
}

// ---- the launchers and the cohort's records: what is launched, with its arguments; the scripted device answers
static std::string P(const void *p) { return rec::tag(p); }
static std::string first_pass_args(const int *desc, double *Sm, int *knn, int *lab, int *out, const int *dims, int nd, int nd_sub)
{ return "desc " + P(desc) + " Sm " + P(Sm) + " knn " + P(knn) + " labels " + P(lab) + " out " + P(out) + " dims " + P(dims) + " clusters " + rec::num(nd) + " coordinates " + rec::num(nd_sub); }
static std::string level_args(const int *desc, const double *Sm, const int *pool, int *knn, int *lab, int *out, int nb, int mmax)
{ return "desc " + P(desc) + " Sm " + P(Sm) + " pool " + P(pool) + " knn " + P(knn) + " labels " + P(lab) + " out " + P(out) + " parts " + rec::num(nb) + " largest " + rec::num(mmax); }
static Cohort::Rec rec_clus1(const PcState &S, int *desc, double *Sm, int *knn, int *lab, int *out, const int *dims, int nd, int nmax, int nd_sub)
{
    const PcState s = S;
    return {"first pass: " + first_pass_args(desc, Sm, knn, lab, out, dims, nd, nd_sub) + " largest " + rec::num(nmax), [=] { devs::first_pass(&s, desc, nd, lab, out, nd_sub > 0); }};
}
static Cohort::Rec rec_clusg(const PcState &S, int *desc, double *Sm, int *pool, int *knn, int *lab, int *out, int nb, int mmax)
{
    const PcState s = S;
    return {"level: " + level_args(desc, Sm, pool, knn, lab, out, nb, mmax), [=] { devs::level(&s, desc, nb, pool, lab, out); }};
}
extern "C" {
int pc_launch_knn_cluster_batch(const PcState *S, const int *h_desc, const int *d_desc, int nd, double *Sm, int *knn, int *labels, int *out, const int *dims, int ndims, hipStream_t)
{
    rec::line("launch first pass: " + first_pass_args(d_desc, Sm, knn, labels, out, dims, nd, ndims) + " host descriptors " + rec::hex(fnv(h_desc, sizeof(int) * 4 * (size_t)nd)));
    devs::first_pass(S, d_desc, nd, labels, out, ndims > 0);
    return 0;
}
int pc_launch_knn_cluster_sub(const int *d_desc, int nb, int mmax, const double *Sm, const int *pool, int *knn, int *labels, int *out, hipStream_t)
{
    rec::line("launch level: " + level_args(d_desc, Sm, pool, knn, labels, out, nb, mmax));
    devs::level(&rec::eng->S, d_desc, nb, pool, labels, out);
    return 0;
}
void pc_launch_remap_chains(const PcState *, const int *map, int nold, int n, hipStream_t) { rec::line("launch remap_chains: map " + P(map) + " clusters " + rec::num(nold) + " chains " + rec::num(n)); }
void pc_launch_shift_mats(const PcState *, int p, int nc, hipStream_t) { rec::line("launch shift_mats: cluster " + rec::num(p) + " of " + rec::num(nc)); }
void pc_launch_rebuild(const PcState *S, int nc, hipStream_t) { rec::line("launch rebuild: clusters " + rec::num(nc)); devs::rebuild(S, nc); }
void pc_launch_ph_rehome(const PcState *S, int nph, int nc, const unsigned *old_uids, int nold_uids, int *counts, hipStream_t)
{
    rec::line("launch ph_rehome: phantoms " + rec::num(nph) + " clusters " + rec::num(nc) + " old ids " + P(old_uids) + " x " + rec::num(nold_uids) + " counts " + P(counts));
    devs::ph_rehome(S, nph, nc, counts);
}
}

// ---- the scenarios
// a cluster of n points; the point at position i carries the digits (i / (fan[0] * .. * fan[l-1])) % fan[l], one per entry of fan (sub: in the sub-dimension pass)
struct ClusterSpec { int n; std::vector<int> fan, sub; };
struct Scenario {
    std::vector<ClusterSpec> cl; int maxc = 16;
    bool two_pass = false, sizes_given = true; int epoch_discard = 0, i_nursery = 0, inject = 0;
};
static bool dump = false;
static std::vector<int> digits(int i, const std::vector<int> &fan)
{
    std::vector<int> d((size_t)devs::PATH, 0);
    for (size_t l = 0; l < fan.size() && l < (size_t)devs::PATH; ++l) { d[l] = i % fan[l]; i /= fan[l]; }
    return d;
}
static double val(unsigned a, unsigned b) { return -(double)(mix(a, b) % 100000u) / 7919.0; }
static void drive(const Scenario &sc, bool in_step)
{
    Engine e; Cohort cohort;
    rec::eng = &e; rec::blocks.clear();
    if (in_step) e.co = &cohort;
    const int nc = (int)sc.cl.size(), maxc = sc.maxc;
    int N = 0; for (const ClusterSpec &c : sc.cl) N += c.n;
    const int Ncap = N + N / 6 + 3;
    PcState &S = e.S;
    S.Ncap = Ncap; S.N = N; S.maxc = maxc; S.D = 4;
    S.live_cluster = dalloc<int>(Ncap); S.live_pos = dalloc<int>(Ncap); S.cl_list = dalloc<int>((size_t)maxc * Ncap); S.cl_n = dalloc<int>(maxc);
    S.logXp = dalloc<double>(maxc); S.logZXp = dalloc<double>(maxc); S.logZp = dalloc<double>(maxc); S.logZp2 = dalloc<double>(maxc); S.logZpXp = dalloc<double>(maxc);
    S.death_thr = dalloc<double>(maxc); S.XpXq = dalloc<double>(2 * (size_t)maxc * maxc); S.cl_uid = dalloc<unsigned>(maxc); S.ctl = dalloc<PcCtl>(1);
    // the clusters' points interleaved over the slots, every seventh slot empty
    devs::path[0].clear(); devs::path[1].clear();
    std::vector<int> left(nc), pos(nc, 0);
    for (int c = 0; c < nc; ++c) left[c] = sc.cl[c].n;
    for (int s = 0, c = 0; s < Ncap; ++s) {
        S.live_cluster[s] = -1; S.live_pos[s] = 0;
        if (s % 7 == 6 || std::all_of(left.begin(), left.end(), [](int l) { return l == 0; })) continue;
        while (left[c % nc] == 0) ++c;
        const int k = c++ % nc;
        S.live_cluster[s] = k; S.live_pos[s] = pos[k];
        devs::path[0][s] = digits(pos[k], sc.cl[k].fan); devs::path[1][s] = digits(pos[k], sc.cl[k].sub);
        pos[k]++; left[k]--;
    }
    devs::rebuild(&S, nc);
    for (int c = 0; c < nc; ++c) {
        S.logXp[c] = val(c, 1); S.logZXp[c] = val(c, 2); S.logZp[c] = val(c, 3); S.logZp2[c] = val(c, 4); S.logZpXp[c] = val(c, 5); S.death_thr[c] = val(c, 6); S.cl_uid[c] = 100u + c;
        for (int q = 0; q < nc; ++q) S.XpXq[(size_t)c * maxc + q] = val(std::min(c, q) * 64 + std::max(c, q), 7);
    }
    PcCtl ctl; std::memset(&ctl, 0, sizeof ctl);
    ctl.ncluster = nc; ctl.nphantom = 37; ctl.next_cluster_uid = 100u + nc; ctl.i_nursery = sc.i_nursery; ctl.admin_epoch = 3;
    e.h_ctl = &ctl; e.cfg.epoch_discard = sc.epoch_discard; e.ncluster_peak = nc;
    const std::vector<int> sub = {0, 2};
    if (sc.two_pass) { e.sub_dims = sub; e.c_subdims = dalloc<int>(sub.size()); std::copy(sub.begin(), sub.end(), e.c_subdims); }
    g_inject_fault = sc.inject;
    // (as Engine::do_update: the clusters' sizes come with the update's own wait)
    std::vector<int> cn;
    if (sc.sizes_given) cn.assign(S.cl_n, S.cl_n + nc);
    std::vector<int> map;
    try {
        if (!sc.two_pass) {
            const bool found = CLUS(e).do_clustering(cn);
            rec::line(std::string("found: ") + (found ? "yes" : "no"));
        } else {
            // nested_sampling.F90:352-367: the sub-dimension pass, then the full one over every cluster there is after it
            std::vector<int> map2;
            bool found = CLUS(e).do_clustering(cn, e.c_subdims, (int)e.sub_dims.size(), &map);
            rec::line(std::string("sub-dimension pass found: ") + (found ? "yes" : "no"));
            if (found) cn.clear();
            found = CLUS(e).do_clustering(cn, nullptr, 0, &map2) || found;
#ifdef SPLIT_PARENT
            for (int &m : map) m = m >= 0 ? map2[(size_t)m] : -1;
#else
            cluster_map_compose(map, map2);
#endif
            if (found && !e.cfg.epoch_discard) CLUS(e).remap_nursery(map, nc);
            rec::line(std::string("found: ") + (found ? "yes" : "no"));
        }
    } catch (const EngineError &err) { rec::line("failed with code " + rec::num(err.code) + ": " + err.msg); }
    if (in_step) rec::line("left written down: " + rec::num((long long)cohort.pend.size()));
    std::string m; for (int v : map) m += " " + rec::num(v);
    rec::line("map:" + m);
    rec::line("clusters " + rec::num(ctl.ncluster) + " peak " + rec::num(e.ncluster_peak) + " room " + rec::num(S.maxc) + " splits " + rec::num(e.nsplits) + " next id " + rec::num(ctl.next_cluster_uid) +
              " epoch " + rec::num(ctl.admin_epoch) + " status " + rec::num(ctl.status));
    std::string g;
    for (size_t k = 0; k < e.split_child.size(); ++k) g += " " + rec::num(e.split_child[k]) + "<" + rec::num(e.split_parent[k]) + ":" + rec::hex(fnv(&e.split_logfrac[k], 8));
    rec::line("genealogy:" + g);
    // what the device holds at the end: labels, lists, the per-cluster arrays and the cross-volume rows of the clusters there are
    unsigned long long h = fnv(S.live_cluster, sizeof(int) * Ncap); h = fnv(S.live_pos, sizeof(int) * Ncap, h);
    for (double *p : {S.logXp, S.logZXp, S.logZp, S.logZp2, S.logZpXp, S.death_thr}) h = fnv(p, sizeof(double) * ctl.ncluster, h);
    h = fnv(S.cl_uid, sizeof(unsigned) * ctl.ncluster, h); h = fnv(S.cl_n, sizeof(int) * ctl.ncluster, h);
    for (int c = 0; c < ctl.ncluster; ++c) h = fnv(S.XpXq + (size_t)c * S.maxc, sizeof(double) * ctl.ncluster, h);
    rec::line("device state " + rec::hex(h));
    g_inject_fault = 0;
#ifndef SPLIT_PARENT
    e.blocks.release_all();
#endif
    for (auto &b : rec::blocks) std::free((void *)b.first);      // (the scenario's device: the state's arrays, and the parent's scratch)
    rec::blocks.clear();
}
static void scenario(const std::string &name, const Scenario &sc)
{
    for (bool in_step : {false, true}) {
        rec::text.clear();
        drive(sc, in_step);
        long lines = 0; for (char ch : rec::text) lines += ch == '\n';
        std::printf("%s%s %016llx %ld\n", name.c_str(), in_step ? "_in_step" : "", fnv(rec::text.data(), rec::text.size()), lines);
        if (dump) std::printf("%s", rec::text.c_str());
    }
}

#ifndef SPLIT_PARENT
// ---- the order of the recursion.  The rule: a part of more than k points splits into 2 ... 4 groups by a hash of its smallest index
static int hash_once(const std::vector<int> &pts, int k, unsigned seed, std::vector<int> &lab)
{
    lab.assign(pts.size(), 1);
    if ((int)pts.size() <= k) return 1;
    const unsigned lo = (unsigned)*std::min_element(pts.begin(), pts.end()), g = 2u + mix(lo, seed) % 3u;
    std::vector<unsigned> seen;
    for (size_t a = 0; a < pts.size(); ++a) {
        const unsigned d = mix((unsigned)pts[a] * 2654435761u + lo, seed) % g;
        size_t f = std::find(seen.begin(), seen.end(), d) - seen.begin();
        if (f == seen.size()) seen.push_back(d);
        lab[a] = (int)f + 1;
    }
    return (int)seen.size();
}
static int relabel_by_first_appearance(std::vector<int> &lab)
{   // utils.F90:713-749
    std::vector<int> seen;
    for (int &l : lab) {
        size_t f = std::find(seen.begin(), seen.end(), l) - seen.begin();
        if (f == seen.size()) seen.push_back(l);
        l = (int)f + 1;
    }
    return (int)seen.size();
}
// NN_clustering with its recursion over the clusters it finds, one after the other, depth first (clustering.f90:80-95)
static int depth_first(const std::vector<int> &pts, int k, unsigned seed, std::vector<int> &labels)
{
    int num = hash_once(pts, k, seed, labels);
    if (pts.size() <= 1) return 1;
    if (num > 1) {
        int ic = 1;
        while (ic <= num) {
            std::vector<int> at, sub, sl;
            for (size_t j = 0; j < pts.size(); ++j) if (labels[j] == ic) { at.push_back((int)j); sub.push_back(pts[j]); }
            const int nnew = depth_first(sub, k, seed, sl);
            for (size_t a = 0; a < at.size(); ++a) labels[(size_t)at[a]] = num + sl[a];
            if (nnew == 1) ic++;
            num = relabel_by_first_appearance(labels);
        }
    }
    return num;
}
static int order_mode()
{
    int tried = 0, wrong = 0;
    for (unsigned seed = 1; seed <= 300; ++seed) {
        // an update's clusters: one to four of 3 ... 200 points, their points numbered as positions in the cluster's order
        const int ncl = 1 + (int)(mix(seed, 11) % 4u), k = 1 + (int)(mix(seed, 12) % 6u);
        std::vector<int> cn;
        for (int c = 0; c < ncl; ++c) cn.push_back(3 + (int)(mix(seed, 20 + c) % 198u));
        const FirstPass fp = first_pass_descriptors(cn);
        std::vector<int> out, lab0((size_t)fp.o1);
        for (int c = 0; c < fp.nd(); ++c) {
            std::vector<int> all((size_t)cn[c]), lab; for (int i = 0; i < cn[c]; ++i) all[i] = i;
            out.push_back(hash_once(all, k, seed * 8 + c, lab));
            std::copy(lab.begin(), lab.end(), lab0.begin() + fp.desc[4 * c + 3]);
        }
        PartRefiner parts; parts.open(fp, out, lab0);
        while (parts.work_left()) {
            const PartRefiner::Level &lev = parts.next_level();
            std::vector<int> labs(lev.pool.size()), nums;
            for (int b = 0; b < lev.nb; ++b) {
                const int *g = &lev.gdesc[5 * b];
                int c = 0; while (fp.desc[4 * c + 2] != g[0]) ++c;
                std::vector<int> pts(lev.pool.begin() + g[2], lev.pool.begin() + g[2] + g[3]), lab;
                nums.push_back(hash_once(pts, k, seed * 8 + c, lab));
                std::copy(lab.begin(), lab.end(), labs.begin() + g[2]);
            }
            parts.take(labs, nums);
        }
        std::vector<std::vector<int>> fl((size_t)ncl); std::vector<int> fn((size_t)ncl, 1);
        parts.finish(fl, fn);
        for (int c = 0; c < ncl; ++c) {
            std::vector<int> all((size_t)cn[c]), want; for (int i = 0; i < cn[c]; ++i) all[i] = i;
            const int num = depth_first(all, k, seed * 8 + c, want);
            if (fl[c].empty()) fl[c].assign((size_t)cn[c], 1);       // (the first pass found one cluster: nothing to refine)
            tried++;
            if (num != fn[c] || want != fl[c]) { wrong++; std::printf("seed %u cluster %d of %d points: %d parts depth first, %d level by level\n", seed, c, cn[c], num, fn[c]); }
        }
    }
    std::printf("order: %d clusters, %d mismatches\n", tried, wrong);
    return wrong != 0;
}
// ---- the pure steps of add_cluster on a fabricated state: cluster 1 of 4 splits into 3
static int split_mode(volatile int *counts /* live and phantom points of the three new clusters */)
{
    const int nc = 4, p = 1, nnew = 3, maxc = 8, Ncap = 12;
    ClusterMirror m; m.size(Ncap, maxc);
    const int lc0[Ncap] = {0, 1, 1, 2, -1, 1, 3, 1, 1, 0, 1, 3}, lp0[Ncap] = {0, 0, 1, 0, 0, 2, 0, 3, 4, 1, 5, 1};
    for (int s = 0; s < Ncap; ++s) { m.lc[s] = lc0[s]; m.lp[s] = lp0[s]; }
    for (int c = 0; c < nc; ++c) {
        m.Xp[c] = val(c, 1); m.ZXp[c] = val(c, 2); m.Zp[c] = val(c, 3); m.Zp2[c] = val(c, 4); m.ZpXp[c] = val(c, 5); m.thr[c] = val(c, 6); m.uid[c] = 10u + c;
        for (int q = 0; q < nc; ++q) m.XQ[(size_t)c * maxc + q] = val(std::min(c, q) * 64 + std::max(c, q), 7);
    }
    auto row = [&](const char *name, const std::vector<double> &v, int n) { std::printf("%s", name); for (int i = 0; i < n; ++i) std::printf(" %a", v[i]); std::printf("\n"); };
    auto rows = [&](const char *name, int n) { for (int a = 0; a < n; ++a) { std::printf("%s %d", name, a); for (int b = 0; b < n; ++b) std::printf(" %a", m.XQ[(size_t)a * maxc + b]); std::printf("\n"); } };
    auto ints = [&](const char *name, const std::vector<int> &v) { std::printf("%s", name); for (int x : v) std::printf(" %d", x); std::printf("\n"); };
    std::printf("split cluster %d of %d into %d\n", p, nc, nnew);
    row("in Xp", m.Xp, nc); row("in ZXp", m.ZXp, nc); row("in Zp", m.Zp, nc); row("in Zp2", m.Zp2, nc); row("in ZpXp", m.ZpXp, nc); rows("in XQ", nc);
    const std::vector<int> labels = {2, 1, 2, 3, 1, 2};      // of the parent's six points, in its point order
    unsigned next_uid = 50;
    const SplitParent par = add_cluster_relabel(m, nc, p, labels, nnew, next_uid);
    ints("lc", m.lc); ints("lp", m.lp);
    std::printf("uid"); for (int c = 0; c < nc + nnew - 1; ++c) std::printf(" %u", m.uid[c]); std::printf(" next %u\n", next_uid);
    row("thr", m.thr, nc + nnew - 1);
    std::vector<int> nlv(nc + nnew - 1, 0), nph(nc + nnew - 1, 0);
    for (int k = 0; k < nnew; ++k) { nlv[nc - 1 + k] = counts[2 * k]; nph[nc - 1 + k] = counts[2 * k + 1]; }
    ints("nlv", std::vector<int>(nlv.begin() + nc - 1, nlv.end())); ints("nph", std::vector<int>(nph.begin() + nc - 1, nph.end()));
    std::vector<unsigned> child, parent; std::vector<double> frac;
    add_cluster_evidence(m, par, nc, p, nnew, nlv, nph, child, parent, frac);
    const int ncn = nc + nnew - 1;
    row("out Xp", m.Xp, ncn); row("out ZXp", m.ZXp, ncn); row("out Zp", m.Zp, ncn); row("out Zp2", m.Zp2, ncn); row("out ZpXp", m.ZpXp, ncn); rows("out XQ", ncn);
    std::printf("genealogy"); for (size_t k = 0; k < child.size(); ++k) std::printf(" %u %u %a", child[k], parent[k], frac[k]); std::printf("\n");
    return 0;
}
#endif

int main(int argc, char **argv)
{
    dump = argc > 1 && !std::strcmp(argv[1], "--dump");
#ifndef SPLIT_PARENT
    if (argc > 1 && !std::strcmp(argv[1], "--order")) return order_mode();
    if (argc > 1 && !std::strcmp(argv[1], "--split")) {
        static volatile int counts[6] = {2, 11, 3, 0, 1, 40};
        for (int k = 0; k < 6 && k + 2 < argc; ++k) counts[k] = std::atoi(argv[k + 2]);
        return split_mode(counts);
    }
#endif
    typedef ClusterSpec C;
    auto of = [](std::vector<ClusterSpec> cl) { Scenario sc; sc.cl = cl; return sc; };
    scenario("nothing_above_two_points", of({C{2, {2}, {}}, C{1, {}, {}}, C{2, {2}, {}}}));
    scenario("one_cluster_not_split", of({C{9, {}, {}}}));
    scenario("one_cluster_in_two", of({C{10, {2}, {}}}));
    scenario("one_cluster_in_five", of({C{23, {5}, {}}}));
    scenario("three_levels_single_points", of({C{7, {2, 2, 2}, {}}}));
    scenario("three_levels_uneven", of({C{29, {3, 2, 2}, {}}, C{5, {}, {}}}));
    scenario("first_and_last_of_three_split", of({C{8, {2}, {}}, C{6, {}, {}}, C{11, {3, 2}, {}}}));
    { Scenario sc = of({C{8, {2}, {}}, C{6, {}, {}}, C{11, {3, 2}, {}}}); sc.sizes_given = false; scenario("sizes_asked_for", sc); }
    for (int nc : {1, 7}) for (int where : {0, 1, 2}) {
        const int p = where == 0 ? 0 : where == 1 ? nc / 2 : nc - 1;
        if (nc == 1 && where) continue;
        std::vector<ClusterSpec> cl;
        for (int c = 0; c < nc; ++c) cl.push_back(c == p ? C{9, {3}, {}} : C{3 + c % 3, {}, {}});
        scenario("split_at_" + std::to_string(p) + "_of_" + std::to_string(nc), of(cl));
    }
    { Scenario sc = of({C{4, {}, {}}, C{12, {4}, {}}, C{9, {2, 2}, {}}}); sc.maxc = 4; scenario("the_list_grows", sc); }
    { Scenario sc = of({C{12, {6}, {}}}); sc.maxc = 2; scenario("the_list_grows_at_the_first_split", sc); }
    for (int which : {1, 2, 3}) {
        Scenario sc = of({C{12, which & 2 ? std::vector<int>{1, 3} : std::vector<int>{}, which & 1 ? std::vector<int>{2} : std::vector<int>{}}, C{7, {}, {}},
                          C{10, which & 2 ? std::vector<int>{2} : std::vector<int>{}, {}}});
        sc.two_pass = true; sc.i_nursery = 5;
        scenario(std::string("two_passes_split_in_") + (which == 1 ? "the_first" : which == 2 ? "the_second" : "both"), sc);
    }
    { Scenario sc = of({C{12, {}, {}}, C{7, {}, {}}}); sc.two_pass = true; sc.i_nursery = 5; scenario("two_passes_no_split", sc); }
    { Scenario sc = of({C{12, {1, 3}, {2}}, C{7, {}, {}}}); sc.two_pass = true; sc.i_nursery = 5; sc.epoch_discard = 1; scenario("two_passes_epoch_discard", sc); }
    for (int discard : {0, 1}) for (int nursery : {0, 9}) {
        Scenario sc = of({C{8, {2}, {}}, C{6, {}, {}}, C{11, {3}, {}}}); sc.epoch_discard = discard; sc.i_nursery = nursery;
        scenario("epoch_discard_" + std::to_string(discard) + "_nursery_" + std::to_string(nursery), sc);
    }
    { Scenario sc = of({C{6, {}, {}}, C{10, {2}, {}}}); sc.inject = 2; scenario("injected_cluster_limit", sc); }
    return 0;
}
