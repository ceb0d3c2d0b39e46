// launch_record.hip -- which kernel the sampling launchers choose, and with what launch shape, recorded on the CPU.
//
// Includes pc_sample.hip and pc_bases.hip (or, with -DRECORD_SLICE_T, pc_slice_t.hip) with hipLaunchKernelGGL and pc_need_dyn_lds turned into
// recorders, and walks a grid of fabricated states through the launchers: no device, no kernel runs.  Built host-only
// (make -C polychordlite_amd/csrc launch_record); tests/test_launch_plan.py compares the digests below with those of the
// commit before the launchers were rewritten around one plan.
//
//   launch_record            one line per launcher: its name, the digest of its record, the number of calls
//   launch_record --kernels  the distinct kernels reached (full template argument lists)
//   launch_record --dump DIR the records themselves, DIR/<launcher>.txt (several hundred MB: for a diff of two builds)
//   launch_record --forms    the second sweep instead of the first: the same launchers over the same grid for source handles of every form
//                            (FORMS below), which is what pins the LDS sizes of pc_launch.h's helpers to the kernels' layout on the CPU
// The developer switches are read once per process: run it once under each of them.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cctype>
#include <string>
#include <set>
#include <vector>
#include "pc_state.h"

namespace rec {
std::string line;                       // the record of the launcher call in progress
std::set<std::string> kernels;
// a kernel's spelling with its full template argument list: k_slice<1, 1, false> is k_slice<1, 1, false, 1, 0, 0, 0>
std::string norm(const char *raw)
{
    std::string s(raw);
    const std::string cast = "(const void *)";
    if (s.compare(0, cast.size(), cast) == 0) s.erase(0, cast.size());
    while (!s.empty() && s.front() == '(' && s.back() == ')') s = s.substr(1, s.size() - 2);
    static const struct { const char *name; std::vector<const char *> dflt; } pad[] = {
        { "k_slice", { nullptr, nullptr, nullptr, "1", "0", "0", "0" } }, { "k_slice_many", { nullptr, nullptr, nullptr, "1", "0", "0" } },
        { "k_generate_live", { nullptr, "0" } }, { "k_nhats", { nullptr, nullptr, "0" } }, { "k_nhats_q", { nullptr, "0" } }, { "k_nhats_q_many", { nullptr, "0" } } };
    const size_t lt = s.find('<');
    if (lt == std::string::npos) return s;
    for (const auto &p : pad) if (s.compare(0, lt, p.name) == 0 && std::strlen(p.name) == lt) {
        size_t n = 1;
        for (char c : s) n += c == ',';
        s.pop_back();
        for (; n < p.dflt.size(); ++n) { s += ", "; s += p.dflt[n]; }
        s += '>';
    }
    return s;
}
// ... and, inside a function template, with the template's parameters replaced by their values (from __PRETTY_FUNCTION__: "... [DT = 5]")
std::string bound(const char *spelling, const char *pretty)
{
    std::string s(spelling);
    const char *lb = std::strrchr(pretty, '[');
    if (!lb || pretty[std::strlen(pretty) - 1] != ']') return norm(s.c_str());
    std::string list(lb + 1, std::strlen(lb) - 2);
    for (size_t at = 0; at < list.size();) {
        size_t end = list.find(", ", at);
        if (end == std::string::npos) end = list.size();
        const std::string item = list.substr(at, end - at);
        const size_t eq = item.find(" = ");
        if (eq != std::string::npos) {
            const std::string name = item.substr(0, eq), val = item.substr(eq + 3);
            auto word = [](char c) { return std::isalnum((unsigned char)c) || c == '_'; };
            for (size_t q = s.find(name); q != std::string::npos; q = s.find(name, q)) {
                if ((q > 0 && word(s[q - 1])) || (q + name.size() < s.size() && word(s[q + name.size()]))) { q += name.size(); continue; }
                s.replace(q, name.size(), val); q += val.size();
            }
        }
        at = end + 2;
    }
    return norm(s.c_str());
}
void launch(const char *k, const char *where, dim3 g, dim3 b, size_t sh)
{
    const std::string n = bound(k, where);
    kernels.insert(n);
    char buf[96];
    std::snprintf(buf, sizeof buf, " g=%u,%u,%u b=%u sh=%zu", g.x, g.y, g.z, b.x, sh);
    line += " | L " + n + buf;
}
void lds(const char *args, const char *where, const void *, size_t sh)
{
    const char *c = std::strrchr(args, ',');
    line += " | A " + bound(std::string(args, c - args).c_str(), where) + " " + std::to_string(sh);
}
struct Launcher {
    const char *name; unsigned long long h = 1469598103934665603ull; long calls = 0; FILE *f = nullptr;
    explicit Launcher(const char *n) : name(n) {}
    void done(const std::string &state, int rc)
    {
        const std::string t = state + " rc=" + std::to_string(rc) + line + "\n";
        for (unsigned char c : t) { h ^= c; h *= 1099511628211ull; }
        if (f) std::fputs(t.c_str(), f);
        ++calls; line.clear();
    }
};
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(K, G, B, SH, ST, ...) rec::launch(#K, __PRETTY_FUNCTION__, G, B, SH)
#define pc_need_dyn_lds(...) rec::lds(#__VA_ARGS__, __PRETTY_FUNCTION__, __VA_ARGS__)

#ifdef RECORD_SLICE_T
#include "pc_slice_t.hip"
#else
#include "pc_sample.hip"
#include "pc_bases.hip"
// what their host code calls in other files
extern "C" int pc_rtc_launch(const PcState *, const char *expr, dim3 grid, dim3 block, size_t sh, hipStream_t, void **) { rec::launch(expr, "", grid, block, sh); return 0; }
// the handles of the two sweeps by src_id -- the first sweep knows 1 (the plain form) and 2 (100 terms) --: nterms, nsums, nquad, nshared
static const PcSourceForm FORMS[] = { {}, {}, {100}, {100, 5}, {100, 8}, {5, 0, 5}, {1024, 0, 1024}, {100, 0, 0, 1}, {100, 0, 0, 512}, {65, 0, 65, 65}, {100, 5, 0, 65} };
static const int NFORMS = sizeof FORMS / sizeof FORMS[0];
extern "C" int pc_rtc_source_form(int id, PcSourceForm *f) { *f = id >= 0 && id < NFORMS ? FORMS[id] : PcSourceForm{}; return 0; }
extern "C" int pc_launch_bases_t(const PcState *S, unsigned, int, hipStream_t) { rec::line += " | bases_t"; return S->D < 2; }
#endif
extern "C" void pc_abi_set_last_error(const char *msg) { if (msg) { rec::line += " | error: "; rec::line += msg; } }

int main(int argc, char **argv)
{
    static double dummy[4];
    static const PcManyRec *dR = (const PcManyRec *)dummy;      // (never read: the kernels are not launched)
    const char *dump = nullptr;
    bool forms = false, list = false;
    for (int a = 1; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--dump") && a + 1 < argc) dump = argv[++a];
        else if (!std::strcmp(argv[a], "--forms")) forms = true;
        else if (!std::strcmp(argv[a], "--kernels")) list = true;
    }
#ifdef RECORD_SLICE_T
    rec::Launcher L[] = { rec::Launcher("slice_t"), rec::Launcher("slice_t_many"), rec::Launcher("slice_t_ok"), rec::Launcher("bases_t"), rec::Launcher("bases_t_many") };
#else
    rec::Launcher L[] = { rec::Launcher("slice"), rec::Launcher("slice_fused"), rec::Launcher("slice_many0"), rec::Launcher("slice_many1"), rec::Launcher("nhats"),
                          rec::Launcher("nhats_part1"), rec::Launcher("nhats_part2"), rec::Launcher("nhats_part1_packed"), rec::Launcher("nhats_many"),
                          rec::Launcher("generate_live"), rec::Launcher("prior_transform"), rec::Launcher("source_eval") };
#endif
    if (dump) for (auto &l : L) { l.f = std::fopen((std::string(dump) + "/" + l.name + ".txt").c_str(), "w"); if (!l.f) { std::perror(dump); return 2; } }
    char st[256];
#ifdef RECORD_SLICE_T
    // lane = chain: every nDims the dispatch knows and one it refuses; decks and records on both sides of 48 and 64 KB of LDS
    // (with and without the helping wavefronts' buffer); grid x runs on both sides of the helpers' limit
    const int nrs[] = {1, 5, 40, 64, 200, 255, 256}, nDers[] = {0, 2, 40, 70}, Rs[] = {1, 3, 16, 64}, nchs[] = {30, 64, 1000, 5000};
    for (int D = 1; D <= 25; ++D) for (int nr : nrs) for (int nDer : nDers) for (int kind : {PC_LIKE_GAUSSIAN, PC_LIKE_RASTRIGIN}) for (int pk = 0; pk <= 2; pk += 2)
    for (int flags = 0; flags < 32; ++flags) {
        PcState S{};
        S.D = D; S.nr = nr; S.nDer = nDer; S.nT = 2 * D + nDer + 2; S.like.kind = kind; S.prior.kind = pk; S.nb_total = (nr + D - 1) / D;
        S.ngrade = (flags & 1) ? 2 : 1; S.seq_mode = (flags & 2) ? 1 : 0; S.ablate = (flags & 4) ? 1 : 0; S.nhat_raw = (flags & 8) ? nullptr : dummy;
        if (flags & 16) { S.prior.lo = dummy; S.prior.hi = dummy; }
        const int len = std::snprintf(st, sizeof st, "D=%d nr=%d nDer=%d kind=%d pk=%d fl=%d", D, nr, nDer, kind, pk, flags);
        for (int ncl = 1; ncl <= 2; ++ncl) { std::snprintf(st + len, sizeof st - len, " ncl=%d", ncl); L[2].done(st, pc_slice_t_ok(&S, ncl)); }
        for (int nch : nchs) {
            std::snprintf(st + len, sizeof st - len, " nch=%d", nch);
            L[0].done(st, pc_launch_slice_t(&S, 7u, nch, nullptr));
            L[3].done(st, pc_launch_bases_t(&S, 7u, nch, nullptr));
            for (int R : Rs) {
                std::snprintf(st + len, sizeof st - len, " nch=%d R=%d", nch, R);
                L[1].done(st, pc_launch_slice_t_many(&S, dR, R, 7u, nch, nullptr));
                L[4].done(st, pc_launch_bases_t_many(&S, dR, R, 7u, nch, nullptr));
            }
        }
    }
#else
    // lane = coordinate: nDims and num_repeats on both sides of every boundary the launchers test (theta rows of the babies on both sides
    // of 48 KB, the fused block and the inverse covariance on both sides of 150 KB), every likelihood kind (a source with and without
    // the terms form), box and table prior, grades, the sequential stream, settings.ablate bits 0 and 13, bases and matrix products
    // in HBM or not, nurseries of a multiple of four chains and not
    const int Ds[] = {1, 8, 9, 16, 17, 20, 24, 25, 32, 33, 64, 65, 80, 96, 112, 113, 128, 129, 256, 257};
    const int nrs[] = {1, 5, 40, 64, 65, 200, 255, 256, 1024, 1025};
    const int kinds[] = {PC_LIKE_CALLBACK, PC_LIKE_GAUSSIAN, PC_LIKE_RASTRIGIN, PC_LIKE_TWIN_GAUSSIAN, PC_LIKE_CORR_GAUSSIAN, PC_LIKE_SOURCE, -PC_LIKE_SOURCE};
    // --forms: a source of every handle of FORMS from 2 on instead of the kinds -- terms, 5 and 8 sums, nres 5 and 1024, nshared 1 and 512 beside
    // terms, shared beside a quadratic form and beside sums.  For the handles whose own block counts in pc_slice_phi_lds's 48 KB decision (several
    // sums, nres = 1024; not a shared handle, which never takes that pass) the sweep must hold states on both sides of the limit: `in`, the babies'
    // rows fit beside the block; `over`, they would fit without it
    std::vector<int> subjects;
    if (forms) for (int h = 2; h < NFORMS; ++h) subjects.push_back(-h); else subjects.assign(kinds, kinds + sizeof kinds / sizeof kinds[0]);
    long in[NFORMS] = {}, over[NFORMS] = {};
    for (int D : Ds) for (int nr : nrs) for (int kind : subjects) for (int nDer = 0; nDer <= 2; nDer += 2) for (int pk = 0; pk <= 2; pk += 2)
    for (int flags = 0; flags < 64; ++flags) for (int nch : {30, 32}) {
        PcState S{};
        S.D = D; S.nr = nr; S.nDer = nDer; S.nT = 2 * D + nDer + 2; S.like.kind = kind < 0 ? PC_LIKE_SOURCE : kind;
        S.src_id = forms ? -kind : (kind == PC_LIKE_SOURCE ? 1 : (kind < 0 ? 2 : 0));
        if (forms && nDer > 0) {
            const PcSourceForm &F = FORMS[S.src_id];
            const size_t rows = sizeof(double) * ((size_t)D + nr) + 16 + sizeof(double) * (size_t)nr * (D + 1);
            const size_t own = sizeof(double) * (size_t)nr * F.nsums + 2 * sizeof(double) * (size_t)((F.nquad + 1) & ~1L);
            if (rows + own <= 48 * 1024) in[S.src_id]++; else if (rows <= 48 * 1024) over[S.src_id]++;
        }
        S.prior.kind = pk; S.nb_total = 2;
        S.ngrade = (flags & 1) ? 2 : 1; S.seq_mode = (flags & 2) ? 1 : 0; S.ablate = ((flags & 4) ? 1 : 0) | ((flags & 8) ? 8192 : 0);
        S.nhat_raw = (flags & 16) ? nullptr : dummy; S.nhat_Ms = (flags & 32) ? dummy : nullptr;
        std::snprintf(st, sizeof st, "D=%d nr=%d kind=%d src=%d nDer=%d pk=%d fl=%d nch=%d", D, nr, S.like.kind, S.src_id, nDer, pk, flags, nch);
        L[0].done(st, pc_launch_slice(&S, 7u, nch, nullptr));
        L[1].done(st, pc_launch_slice_fused(&S, 7u, nch, nullptr));
        L[2].done(st, pc_launch_slice_many(&S, dR, 3, nch, 0, nullptr));
        L[3].done(st, pc_launch_slice_many(&S, dR, 3, nch, 1, nullptr));
        L[4].done(st, pc_launch_nhats(&S, 7u, nch, nullptr));
        L[5].done(st, pc_launch_nhats_part(&S, 7u, nch, 1, nullptr, 0));
        L[6].done(st, pc_launch_nhats_part(&S, 7u, nch, 2, nullptr, 0));
        L[7].done(st, pc_launch_nhats_part(&S, 7u, nch, 1, nullptr, 1));
        L[8].done(st, pc_launch_nhats_many(&S, dR, 3, nch, nullptr));
        L[9].done(st, pc_launch_generate_live(&S, 0, 50, nullptr, nullptr, nullptr));
        L[10].done(st, pc_launch_prior_transform(&S, 50, nullptr, nullptr, nullptr));
        L[11].done(st, pc_launch_source_eval(&S, 50, nullptr, nullptr, nullptr, nullptr));
    }
    for (int h : {3, 4, 6}) if (forms && !(in[h] && over[h])) { std::fprintf(stderr, "--forms: handle %d has no state on both sides of the 48 KB limit (%ld, %ld)\n", h, in[h], over[h]); return 1; }
#endif
    if (list) { for (const auto &k : rec::kernels) std::printf("%s\n", k.c_str()); return 0; }
    for (auto &l : L) { std::printf("%s %016llx %ld\n", l.name, l.h, l.calls); if (l.f) std::fclose(l.f); }
    return 0;
}
