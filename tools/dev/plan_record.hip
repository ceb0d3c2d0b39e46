// plan_record.hip -- the decisions of pc_plan.h against the conditions they replaced, on the CPU, over the full grid of their facts.
//
// Host only (make -C polychordlite_amd/csrc plan_record): includes pc_plan.h, launches nothing.  The functions old_*() below are the conditions of
// ba2108c's pc_engine.hip -- the commit before pc_plan.h existed -- transcribed one function per decision, each condition with its line number
// there; the six environment switches that duplicated a settings.ablate bit (removed with that commit's successor) are taken as unset.  They are the
// reference tests/test_run_plan.py compares with, so they stay here.
//
//   plan_record            one line per decision: its name, the digest of the new answers, the digest of the transcribed parent's, the grid points, the
//                          points where the two differ; then one line per enumerator of every choice: how many grid points chose it
//   plan_record --dump     also the grid points where old and new differ (the first 200 of a decision)
// An answer = the choice, what goes with it, and its pchip_result.path[] increments.
//
// The grid: every boolean fact both ways; ncluster in {0, 1, 2, 64, 65}; nDims in {8, 24, 25, 64, 65, 128, 129}; nursery_left in {0, 1, 2}; phantom rows
// in {0, 1}; force_general in {0, 1, 2}; settings.ablate 0 and each of the plan's bits (1, 2, 3, 5, 6, 7) alone.
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <string>
#include <vector>
#include "pc_plan.h"

namespace {
const int ABLATES[] = {0, 1 << 1, 1 << 2, 1 << 3, 1 << 5, 1 << 6, 1 << 7};
const int NCLUSTERS[] = {0, 1, 2, 64, 65}, DIMS[] = {8, 24, 25, 64, 65, 128, 129}, LEFTS[] = {0, 1, 2}, FORCE[] = {0, 1, 2};
bool g_dump = false;

// an answer as integers: compared, digested, printed
struct Answer {
    std::vector<long> v;
    void add(long x) { v.push_back(x); }
    void add_paths(const long *path) { for (int k = 0; k < PCHIP_PATH_COUNT; ++k) v.push_back(path[k]); }
};
struct Decision {
    const char *name; uint64_t h_new = 1469598103934665603ull, h_old = 1469598103934665603ull; long points = 0, differ = 0;
    static void mix(uint64_t &h, const Answer &a) { for (long x : a.v) { h ^= (uint64_t)x; h *= 1099511628211ull; } h ^= 0xFFu; h *= 1099511628211ull; }
    void take(const Answer &nw, const Answer &old, const std::string &where)
    {
        mix(h_new, nw); mix(h_old, old); points++;
        if (nw.v != old.v) {
            if (g_dump && differ < 200) {
                std::printf("differs %s: %s\n    new", name, where.c_str());
                for (long x : nw.v) std::printf(" %ld", x);
                std::printf("\n    old");
                for (long x : old.v) std::printf(" %ld", x);
                std::printf("\n");
            }
            differ++;
        }
    }
    void print() const { std::printf("%s %016llx %016llx %ld %ld\n", name, (unsigned long long)h_new, (unsigned long long)h_old, points, differ); }
};

// ---- the settings of a run as ba2108c's begin() and do_update() saw them
struct OldRun {
    int ablate, force_general; bool n_nlives0, nprior_ok, resume_static, par_fits, fast_fits, fused_fits_one, do_clustering, boost, dumper, on_update, resume_write,
        seq_mode, posteriors, equals, callback_mode;
};
struct OldPlan { bool static_ok, fast_ok, par_ok, cl_gate, defer, pool; };
OldPlan old_run(const OldRun &c)
{
    OldPlan o;
    o.static_ok = c.n_nlives0 && c.nprior_ok && c.resume_static && c.force_general != 1;                                         // 2102
    o.fast_ok = o.static_ok && c.fast_fits;                                                                                    // 2103
    o.par_ok = o.static_ok && c.force_general == 0 && c.par_fits;                                                              // 2104
    o.defer = !(c.ablate & 4) && o.par_ok && !c.do_clustering && !c.boost && !c.dumper && !c.on_update && !c.resume_write &&    // 2112
              !c.seq_mode && c.fused_fits_one && !(c.ablate & 8);                                                              // 2113
    o.pool = o.defer && !c.callback_mode && !(c.ablate & 2);                                                                   // 2118
    o.cl_gate = o.static_ok && c.force_general == 0 && !(c.ablate & 32);                                                       // 2303, 2329
    return o;
}
PcRunFacts facts_of(const OldRun &c)
{
    PcRunFacts f{};
    f.ablate = c.ablate; f.force_general = c.force_general; f.fixed_nlive = c.n_nlives0 && c.nprior_ok && c.resume_static;
    f.par_fits = c.par_fits; f.fast_fits = c.fast_fits; f.fused_fits_one = c.fused_fits_one; f.clustering = c.do_clustering; f.boost = c.boost;
    f.dumper = c.dumper; f.on_update = c.on_update; f.resume_write = c.resume_write; f.seq_mode = c.seq_mode; f.posteriors = c.posteriors || c.equals;
    f.callback = c.callback_mode;
    return f;
}

// ---- do_update (1246-1316) and finish_may_wait (2372-2377)
Answer old_update(const OldRun &c, int nph, bool fused_fits, int ncluster)
{
    long path[PCHIP_PATH_COUNT] = {};
    const bool seq_post = c.seq_mode && (c.posteriors || c.equals);                                                             // 1250
    const bool ctl_late = c.do_clustering && !(c.dumper || c.on_update || c.resume_write || c.boost || seq_post);                // 1252
    const bool ctl_early = !ctl_late && (c.dumper || c.on_update || c.do_clustering || c.resume_write || c.boost || seq_post);   // 1253
    const bool hook_late = c.boost && (c.posteriors || c.equals);                                                               // 1256 (and 1295: the rows collected)
    const bool fused = !(c.ablate & 8) && nph > 0 && !c.do_clustering && !c.boost && fused_fits;                                 // 1260
    bool need_count;
    if (fused) { path[PCHIP_PATH_UPDATE_FUSED]++; need_count = c.resume_write || c.dumper || c.on_update || seq_post; }          // 1270, 1274
    else { path[PCHIP_PATH_UPDATE_STEPS]++; need_count = c.do_clustering || c.resume_write || c.dumper || c.on_update || c.boost || seq_post; }   // 1288, 1300
    const bool may_wait = c.do_clustering || c.dumper || c.on_update || c.resume_write || c.boost || c.seq_mode || ncluster > 1 || !fused_fits;   // 2375-2376
    Answer a;
    a.add(fused ? PC_UPDATE_FUSED : PC_UPDATE_STEPS); a.add(need_count); a.add(ctl_early ? PC_CTL_EARLY : ctl_late ? PC_CTL_LATE : PC_CTL_NONE); a.add(hook_late); a.add(may_wait);
    a.add_paths(path);
    return a;
}
Answer new_update(const PcRunPlan &p, const PcUpdateFacts &f, long *reached_kind, long *reached_ctl)
{
    long path[PCHIP_PATH_COUNT] = {};
    const PcUpdateChoice c = pc_choose_update(p, f);
    pc_count(path, c);
    reached_kind[c.kind]++; reached_ctl[c.ctl]++;
    Answer a;
    a.add(c.kind); a.add(c.need_count); a.add(c.ctl); a.add(c.hook_late); a.add(c.may_wait);
    a.add_paths(path);
    return a;
}

// ---- enqueue_nursery (2141-2219)
struct OldNursery {
    bool co, other_active, callback_mode, raw_buf1, slot_ready, st2, depth2, splittable_fn, fusable_fn, bases_t, slice_t, cohort_general, rtc, src_terms, prior_table;
    int D, ablate;
};
Answer old_nursery(const OldNursery &n)
{
    long path[PCHIP_PATH_COUNT] = {};
    int bases, sampler, ahead = PC_AHEAD_NONE; bool packed = false, part2 = false;
    const bool multi = n.co || n.other_active;                                                                                  // 2156
    const bool splittable = n.splittable_fn && n.raw_buf1 && !(n.D > 24 && n.D <= 64 && multi);                                  // 2158
    const bool split = splittable && !multi;                                                                                    // 2159
    bool fused_slice = false;                                                                                                   // 2160
    if (splittable) {                                                                                                           // 2162
        if (n.slot_ready) bases = PC_BASES_READY;                                                                               // 2167
        else if (n.co && n.bases_t) bases = PC_BASES_PART1_STEP;                                                                // 2171
        else { bases = PC_BASES_PART1; packed = multi || (n.ablate & 128); }                                                    // 2172
        fused_slice = !n.callback_mode && n.fusable_fn;                                                                         // 2175
        part2 = !fused_slice;                                                                                                   // 2176
    }
    else if (n.co && !n.callback_mode && n.cohort_general && n.D >= 25 && n.D <= 64) bases = PC_BASES_NHATS_G;                   // 2179
    else bases = PC_BASES_WHOLE;                                                                                                // 2180
    if (n.callback_mode) sampler = PC_SAMPLER_CALLBACK;                                                                         // 2183
    else if (fused_slice && (multi || (n.ablate & 64)) && n.slice_t) {                                                          // 2186
        sampler = PC_SAMPLER_LANE;
        path[PCHIP_PATH_SLICE_LANE]++;                                                                                          // 2187
        if (n.co && n.st2 && splittable && n.depth2 && n.bases_t) ahead = PC_AHEAD_STEP;                                        // 2190
    }
    else if (n.co && !n.callback_mode && n.cohort_general && (fused_slice || !splittable)) {                                    // 2192
        sampler = PC_SAMPLER_WAVE_STEP;
        path[PCHIP_PATH_SLICE_WAVE]++;                                                                                          // 2194
        if (n.rtc) path[PCHIP_PATH_SOURCE_KERNELS]++;                                                                           // 2195
        if (fused_slice && n.st2 && n.depth2 && n.bases_t) ahead = PC_AHEAD_STEP;                                               // 2198
    }
    else {
        sampler = PC_SAMPLER_WAVE;
        path[PCHIP_PATH_SLICE_WAVE]++;                                                                                          // 2202
        if (n.rtc) path[PCHIP_PATH_SOURCE_KERNELS]++;                                                                           // 2203
        if (n.src_terms) path[PCHIP_PATH_SOURCE_TERMS]++;                                                                       // 2204
        if (n.prior_table) path[PCHIP_PATH_DEVICE_PRIOR]++;                                                                     // 2205
    }
    if (split) { if (ahead != PC_AHEAD_NONE) ahead = -1; else ahead = PC_AHEAD_SIDE; }                                          // 2213 (-1: both would follow -- never)
    Answer a;
    a.add(bases); a.add(packed); a.add(part2); a.add(sampler); a.add(fused_slice); a.add(ahead);
    a.add_paths(path);
    return a;
}

// ---- round_enqueue (2292-2369)
struct OldContract { int ncluster, nursery_left; bool co, cohort_general, nn_list, nn_off, nn_valid, cl_fits, clp_fits; };
Answer old_contract(const OldRun &c, const OldPlan &o, const OldContract &r)
{
    long path[PCHIP_PATH_COUNT] = {};
    int kind; bool want_nn = false, clp = false;
    const bool use_fast = o.fast_ok && r.ncluster == 1;                                                                         // 2309
    if (o.par_ok && r.ncluster == 1) { kind = PC_CONTRACT_PAR; path[PCHIP_PATH_CONSUME_PAR]++; }                                // 2312, 2315
    else if (use_fast) { kind = PC_CONTRACT_FAST; path[PCHIP_PATH_CONSUME_FAST]++; }                                            // 2319
    else {
        want_nn = r.ncluster > 1 && r.nn_list && !r.nn_valid && !r.nn_off && !c.seq_mode && r.nursery_left > 1;                 // 2325
        const bool use_cl = o.static_ok && c.force_general == 0 && !(c.ablate & 32) && (r.nn_valid || want_nn) && !c.seq_mode && r.ncluster > 1 &&   // 2329
                            r.cl_fits;                                                                                          // 2330
        if (r.co && use_cl && r.cohort_general) {                                                                               // 2331
            kind = PC_CONTRACT_CL_STEP;
            if (want_nn) path[PCHIP_PATH_NN_LISTS]++;                                                                           // 2335
            clp = r.clp_fits; path[clp ? PCHIP_PATH_CONSUME_CL : PCHIP_PATH_CONSUME_CL_SERIAL]++;                               // 2336
        } else {
            if (want_nn) path[PCHIP_PATH_NN_LISTS]++;                                                                           // 2348
            clp = use_cl && r.clp_fits;
            path[use_cl ? (r.clp_fits ? PCHIP_PATH_CONSUME_CL : PCHIP_PATH_CONSUME_CL_SERIAL) : PCHIP_PATH_CONSUME_GENERAL]++;  // 2350
            kind = use_cl ? PC_CONTRACT_CL : PC_CONTRACT_GENERAL;                                                               // 2351
        }
    }
    Answer a;
    a.add(kind); a.add(want_nn); a.add(clp);
    a.add_paths(path);
    return a;
}

const char *const BASES_NAMES[] = {"PC_BASES_READY", "PC_BASES_PART1", "PC_BASES_PART1_STEP", "PC_BASES_NHATS_G", "PC_BASES_WHOLE"};
const char *const SAMPLER_NAMES[] = {"PC_SAMPLER_CALLBACK", "PC_SAMPLER_LANE", "PC_SAMPLER_WAVE_STEP", "PC_SAMPLER_WAVE"};
const char *const AHEAD_NAMES[] = {"PC_AHEAD_NONE", "PC_AHEAD_STEP", "PC_AHEAD_SIDE"};
const char *const CONTRACT_NAMES[] = {"PC_CONTRACT_PAR", "PC_CONTRACT_FAST", "PC_CONTRACT_CL_STEP", "PC_CONTRACT_CL", "PC_CONTRACT_GENERAL"};
const char *const UPDATE_NAMES[] = {"PC_UPDATE_FUSED", "PC_UPDATE_STEPS"};
const char *const CTL_NAMES[] = {"PC_CTL_NONE", "PC_CTL_EARLY", "PC_CTL_LATE"};
template <int N> void print_reached(const char *const (&names)[N], const long (&n)[N]) { for (int k = 0; k < N; ++k) std::printf("reached %s %ld\n", names[k], n[k]); }
std::string bits(std::initializer_list<int> v) { std::string s; for (int x : v) { s += std::to_string(x); s += ' '; } return s; }
}

int main(int argc, char **argv)
{
    g_dump = argc > 1 && !std::strcmp(argv[1], "--dump");
    Decision d_run{"run"}, d_update{"update"}, d_nursery{"nursery"}, d_contract{"contract"};
    long r_bases[5] = {}, r_sampler[4] = {}, r_ahead[3] = {}, r_contract[5] = {}, r_update[2] = {}, r_ctl[3] = {};
    long r_defer[2] = {}, r_pool[2] = {};

    // ---- the run's plan, and with every plan the updates and the contractions
    for (int ablate : ABLATES) for (int fg : FORCE) for (unsigned m = 0; m < (1u << 15); ++m) {
        auto b = [&](int k) { return ((m >> k) & 1u) != 0; };
        const OldRun c{ablate, fg, b(0), b(1), b(2), b(3), b(4), b(5), b(6), b(7), b(8), b(9), b(10), b(11), b(12), b(13), b(14)};
        const OldPlan o = old_run(c);
        const PcRunPlan p = pc_plan_run(facts_of(c));
        Answer an, ao;
        an.add(p.static_ok); an.add(p.fast_ok); an.add(p.par_ok); an.add(p.cl_ok); an.add(p.defer); an.add(p.pool);
        ao.add(o.static_ok); ao.add(o.fast_ok); ao.add(o.par_ok); ao.add(o.cl_gate); ao.add(o.defer); ao.add(o.pool);
        r_defer[p.defer]++; r_pool[p.pool]++;
        const std::string where = g_dump ? "ablate " + std::to_string(ablate) + " force_general " + std::to_string(fg) + " facts " + std::to_string(m) : std::string();
        d_run.take(an, ao, where);
        for (int nph = 0; nph <= 1; ++nph) for (int nc : NCLUSTERS) for (int ff = 0; ff <= 1; ++ff)
            d_update.take(new_update(p, PcUpdateFacts{nph > 0, ff != 0, nc}, r_update, r_ctl), old_update(c, nph, ff != 0, nc),
                          g_dump ? where + " nph " + bits({nph}) + "ncluster " + bits({nc}) + "fused_fits " + bits({ff}) : where);
        // (a contraction asks the plan's gates and the sequential mode only: the run's other facts at one value)
        if ((m >> 5) != 0 && (m >> 5) != (1u << 6)) continue;      // (bits 5 ... 14 clear, or seq_mode -- bit 11 -- alone)
        for (int nc : NCLUSTERS) for (int left : LEFTS) for (unsigned q = 0; q < (1u << 7); ++q) {
            auto g = [&](int k) { return ((q >> k) & 1u) != 0; };
            const OldContract r{nc, left, g(0), g(1), g(2), g(3), g(4), g(5), g(6)};
            // (the facts as Engine::contract_facts makes them)
            PcContractFacts f{};
            f.ncluster = nc; f.nursery_left = left; f.in_step = r.co; f.cohort_general = r.cohort_general; f.nn_lists = r.nn_list && !r.nn_off; f.nn_valid = r.nn_valid;
            f.cl_fits = nc > 1 && r.cl_fits; f.clp_fits = f.cl_fits && r.clp_fits;
            long path[PCHIP_PATH_COUNT] = {};
            const PcContractChoice ch = pc_choose_contract(p, f);
            pc_count(path, ch);
            r_contract[ch.kind]++;
            Answer a; a.add(ch.kind); a.add(ch.want_nn); a.add(ch.clp); a.add_paths(path);
            d_contract.take(a, old_contract(c, o, r), g_dump ? where + " ncluster " + bits({nc}) + "left " + bits({left}) + "facts " + bits({(int)q}) : where);
        }
    }
    // ---- a nursery (of the plan it asks the ablate bits only)
    for (int ablate : ABLATES) for (int D : DIMS) for (unsigned m = 0; m < (1u << 15); ++m) {
        auto b = [&](int k) { return ((m >> k) & 1u) != 0; };
        const OldNursery n{b(0), b(1), b(2), b(3), b(4), b(5), b(6), b(7), b(8), b(9), b(10), b(11), b(12), b(13), b(14), D, ablate};
        PcRunPlan p{}; p.ablate = ablate;
        // (the facts as Engine::nursery_facts makes them)
        PcNurseryFacts f{};
        f.in_step = n.co; f.other_active = n.other_active; f.callback = n.callback_mode; f.D = D; f.ring = n.raw_buf1; f.slot_ready = n.slot_ready;
        f.second_stream = n.co && n.st2 && n.depth2;
        f.splittable = n.splittable_fn; f.fusable = n.fusable_fn; f.bases_t = n.bases_t; f.slice_t = n.slice_t; f.cohort_general = n.cohort_general;
        f.traits = PcLaunchTraits{n.rtc, n.src_terms, n.prior_table};
        long path[PCHIP_PATH_COUNT] = {};
        const PcNurseryChoice ch = pc_choose_nursery(p, f);
        pc_count(path, ch);
        r_bases[ch.bases]++; r_sampler[ch.sampler]++; r_ahead[ch.ahead]++;
        Answer a; a.add(ch.bases); a.add(ch.packed); a.add(ch.part2); a.add(ch.sampler); a.add(ch.fused); a.add(ch.ahead); a.add_paths(path);
        d_nursery.take(a, old_nursery(n), g_dump ? "ablate " + bits({ablate}) + "D " + bits({D}) + "facts " + bits({(int)m}) : std::string());
    }
    d_run.print(); d_update.print(); d_nursery.print(); d_contract.print();
    print_reached(BASES_NAMES, r_bases); print_reached(SAMPLER_NAMES, r_sampler); print_reached(AHEAD_NAMES, r_ahead);
    print_reached(CONTRACT_NAMES, r_contract); print_reached(UPDATE_NAMES, r_update); print_reached(CTL_NAMES, r_ctl);
    std::printf("reached defer %ld\nreached no_defer %ld\nreached pool %ld\nreached no_pool %ld\n", r_defer[1], r_defer[0], r_pool[1], r_pool[0]);
    return (d_run.differ || d_update.differ || d_nursery.differ || d_contract.differ) ? 1 : 0;
}
