// slice_step_record.hip -- what pc_launch_slice_step (pc_sample.hip) accepts, declines and launches, checked on the CPU.
//
// Includes pc_sample.hip (and pc_bases.hip, whose pc_nhats_splittable pc_slice_fusable asks) with hipLaunchKernelGGL and pc_need_dyn_lds turned into recorders, as launch_record.hip does, and walks a grid of
// fabricated states through the launcher: no device, no kernel runs.  Unlike launch_record it compares with nothing recorded earlier (the
// launcher is new): it holds every call against the launcher's rules written down a second time, here --
//   declined (1)   nDims > 64 unfused; fused where pc_slice_fusable says no; more than one grade; the sequential stream; the correlated Gaussian
//   accepted (0)   everything else: ONE launch of a row of PC_SLICE_STEP_VARIANTS, grid (chains, runs), 64 threads, the chain's LDS block plus
//                  nDims doubles for a terms handle (and num_repeats x nsums for one with several sums, where the babies' theta rows are in LDS --
//                  that block counts in the 48 KB decision), pc_need_dyn_lds above 48 KB, LEAN = 0 whatever the likelihood, PT = 1 for prior kinds 2, 3
// Exit code 0 and a summary line when all calls agree; 1 and the first disagreements otherwise.  `--kernels`: the rows reached.
// Built host-only with the address and undefined-behaviour sanitizers on the host code (make -C polychordlite_amd/csrc slice_step_record); tests/test_in_step_device.py runs it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <set>
#include <vector>
#include "pc_state.h"

namespace rec {
struct Launch { std::string kernel; dim3 g, b; size_t sh; };
std::vector<Launch> launches;
std::vector<std::pair<std::string, size_t>> attrs;
std::string error;
std::string strip(const char *raw)
{
    std::string s(raw);
    const std::string cast = "(const void *)";
    if (s.compare(0, cast.size(), cast) == 0) s.erase(0, cast.size());
    while (!s.empty() && s.front() == '(' && s.back() == ')') s = s.substr(1, s.size() - 2);
    return s;
}
void launch(const char *k, dim3 g, dim3 b, size_t sh) { launches.push_back({strip(k), g, b, sh}); }
void lds(const char *args, const void *, size_t sh) { const char *c = std::strrchr(args, ','); attrs.push_back({strip(std::string(args, c - args).c_str()), sh}); }
void clear() { launches.clear(); attrs.clear(); error.clear(); }
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(K, G, B, SH, ST, ...) rec::launch(#K, G, B, SH)
#define pc_need_dyn_lds(...) rec::lds(#__VA_ARGS__, __VA_ARGS__)

#include "pc_sample.hip"
#include "pc_bases.hip"
// what their host code calls in other files
extern "C" int pc_rtc_launch(const PcState *, const char *expr, dim3 grid, dim3 block, size_t sh, hipStream_t, void **) { rec::launch(expr, grid, block, sh); return 0; }
// (handle 1 the plain form, 2 a hundred terms, 3 a hundred terms in five sums; no quadratic form and no shared values here)
extern "C" int pc_rtc_source_form(int id, PcSourceForm *f) { *f = PcSourceForm{}; f->nterms = id == 2 || id == 3 ? 100 : 0; f->nsums = id == 3 ? 5 : 0; return 0; }
extern "C" int pc_launch_bases_t(const PcState *S, unsigned, int, hipStream_t) { return S->D < 2; }
extern "C" void pc_abi_set_last_error(const char *msg) { if (msg) rec::error = msg; }

int main(int argc, char **argv)
{
    static double dummy[4];
    static const PcManyRec *dR = (const PcManyRec *)dummy;      // (never read: the kernels are not launched)
    std::set<std::string> table;
#define PC_ROW(DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT) table.insert("k_slice_many<" #DPL ", " #NROWS ", " #SPECIAL ", " #WPB ", " #FW ", " #LEAN ", " #PT ">");
    PC_SLICE_STEP_VARIANTS(PC_ROW)
#undef PC_ROW
    std::set<std::string> reached;
    long calls = 0, accepted = 0, bad = 0;
    auto fail = [&](const char *st, const std::string &what) { if (bad++ < 20) std::fprintf(stderr, "%s: %s\n", st, what.c_str()); };
    // nDims and num_repeats on both sides of every boundary the launcher tests (the fused widths 8 / 16 / 24, NROWS at 16 / 32, the unfused limit
    // 64; the babies' theta rows on both sides of 48 KB, the fused block on both sides of 150 KB), every likelihood kind (a source without and
    // with the terms form, of one sum and of five), every prior kind, grades, the sequential stream, settings.ablate bits 0 and 15, bases in HBM or not
    const int Ds[] = {1, 2, 8, 9, 16, 17, 20, 24, 25, 32, 33, 64, 65, 128, 256, 257};
    const int nrs[] = {1, 5, 40, 64, 65, 200, 255, 256, 1024, 1025};
    const int kinds[] = {PC_LIKE_GAUSSIAN, PC_LIKE_RASTRIGIN, PC_LIKE_TWIN_GAUSSIAN, PC_LIKE_CORR_GAUSSIAN, PC_LIKE_SOURCE, -PC_LIKE_SOURCE, -100};
    char st[256];
    for (int D : Ds) for (int nr : nrs) for (int kind : kinds) for (int nDer = 0; nDer <= 2; nDer += 2) for (int pk = 1; pk <= 3; ++pk)
    for (int flags = 0; flags < 32; ++flags) for (int R : {1, 3, 16}) for (int nch : {30, 32}) for (int fused = 0; fused <= 1; ++fused) {
        PcState S{};
        S.D = D; S.nr = nr; S.nDer = nDer; S.nT = 2 * D + nDer + 2; S.like.kind = kind < 0 ? PC_LIKE_SOURCE : kind; S.src_id = kind == PC_LIKE_SOURCE ? 1 : (kind == -PC_LIKE_SOURCE ? 2 : (kind < 0 ? 3 : 0));
        S.prior.kind = pk; S.nb_total = 2;
        S.ngrade = (flags & 1) ? 2 : 1; S.seq_mode = (flags & 2) ? 1 : 0; S.ablate = ((flags & 4) ? PC_ABL_FUNCTOR : 0) | ((flags & 8) ? PC_ABL_RTC_BUILTINS : 0);
        S.nhat_raw = (flags & 16) ? nullptr : dummy;
        std::snprintf(st, sizeof st, "D=%d nr=%d kind=%d src=%d nDer=%d pk=%d fl=%d R=%d nch=%d fused=%d", D, nr, S.like.kind, S.src_id, nDer, pk, flags, R, nch, fused);
        rec::clear();
        const int rc = pc_launch_slice_step(&S, dR, R, nch, fused, nullptr);
        ++calls;
        // the rules a second time
        const bool one_grade = S.ngrade <= 1 && !S.seq_mode, corr = S.like.kind == PC_LIKE_CORR_GAUSSIAN;
        bool want = one_grade && !corr && (fused ? pc_slice_fusable(&S) != 0 : D <= 64);
        const int fw = !fused ? 0 : (D <= 8 ? 8 : (D <= 16 ? 16 : 24)), nrows = D <= 16 ? 1 : ((D <= 32 || fused) ? 2 : 4);
        const size_t sums = S.src_id == 3 ? sizeof(double) * (size_t)nr * 5 : 0;
        const bool phi = nDer > 0 && sizeof(double) * ((size_t)D + nr) + 16 + sizeof(double) * (size_t)nr * (D + 1) + sums <= 48 * 1024;
        size_t sh = sizeof(double) * ((size_t)D + nr) + 16 + (phi ? sizeof(double) * (size_t)nr * (D + 1) : 0);
        if (fused) sh += sizeof(double) * ((size_t)fw * D + (size_t)nr * (D + 2));
        if (S.src_id >= 2) sh += sizeof(double) * (size_t)D;
        if (phi) sh += sums;
        if (fused && sh > 150 * 1024) want = false;
        if (fused && want && (D > 24 || nr > 1024 || !S.nhat_raw)) fail(st, "pc_slice_fusable took a shape the fused kernel has no room for");
        if ((rc == 0) != want) { fail(st, std::string(rc == 0 ? "accepted" : "declined") + ", the rules say otherwise"); continue; }
        if (rc != 0) {
            if (!rec::launches.empty() || !rec::attrs.empty()) fail(st, "declined, but something was launched");
            if (!rec::error.empty()) fail(st, "declined with an error text (a plan without a row?): " + rec::error);
            continue;
        }
        ++accepted;
        if (rec::launches.size() != 1) { fail(st, "accepted, but not ONE launch"); continue; }
        const rec::Launch &L = rec::launches[0];
        char name[96];
        std::snprintf(name, sizeof name, "k_slice_many<1, %d, false, 1, %d, 0, %d>", nrows, fw, pk >= 2 ? 1 : 0);
        if (!table.count(L.kernel)) fail(st, "launched " + L.kernel + ", which is no row of PC_SLICE_STEP_VARIANTS");
        if (L.kernel != name) fail(st, "launched " + L.kernel + ", the rules say " + name);
        if (L.g.x != (unsigned)nch || L.g.y != (unsigned)R || L.g.z != 1 || L.b.x != 64 || L.b.y != 1 || L.b.z != 1) fail(st, "grid or block");
        if (L.sh != sh) fail(st, "LDS " + std::to_string(L.sh) + ", the rules say " + std::to_string(sh));
        const bool rtc = S.like.kind == PC_LIKE_SOURCE || (S.ablate & PC_ABL_RTC_BUILTINS);
        (void)rtc;      // (both ways end in rec::launch: the static kernel's name and the module's are the same text)
        if (sh > 48 * 1024 ? (rec::attrs.size() != 1 || rec::attrs[0].first != L.kernel || rec::attrs[0].second != sh) : !rec::attrs.empty()) fail(st, "pc_need_dyn_lds");
        reached.insert(L.kernel);
    }
    if (argc > 1 && !std::strcmp(argv[1], "--kernels")) { for (const auto &k : reached) std::printf("%s\n", k.c_str()); return bad ? 1 : 0; }
    std::printf("%ld calls, %ld accepted, %zu of %zu rows reached, %ld disagreements\n", calls, accepted, reached.size(), table.size(), bad);
    return bad ? 1 : 0;
}
