// pc_rtc.hip -- user likelihoods written as HIP device source, fused into the sampling kernels at run time.
//
// A source (pchip_source_create) is a string that defines
//     __device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);
// The library compiles it with hiprtc, together with the exact text of its own sampling kernels (pc_dev.h, pc_state.h, pc_seed.h,
// pc_sample.hip and pc_slice_body.inc, embedded when the library is built: pc_rtc_sources.inc), for the device a run is on -- the kernels
// that evaluate the user's problem and nothing else: the direction kernels (pc_bases.hip) exist in the library alone.  The launchers of
// pc_sample.hip choose a kernel variant and its launch shape as they do for the built-ins, and hand the variant's name to pc_rtc_launch,
// which instantiates it (hiprtcAddNameExpression), loads the code object once per device and launches it with the same arguments and
// the same dynamic LDS.
//
// The terms form (pchip_source_create_terms): the source defines pchip_logl_term (the i-th term of a sum over the data, one lane per i) and
// pchip_logl_finish (logL and the derived parameters from the finished sum) instead.  The form and the number of terms reach the kernels
// as #defines in front of the library's text in that handle's unit (PCHIP_USER_TERMS, PCHIP_SRC_NTERMS): pc_sample.hip's wave-cooperative
// evaluation is compiled in their place only.
//
// Several sums per evaluation (pchip_source_create_sums): the source defines pchip_logl_terms (the i-th terms of all the sums, one lane per i)
// and pchip_logl_finish_sums (logL and the derived parameters from the finished sums); such a handle's unit gets PCHIP_USER_SUMS and
// PCHIP_SRC_NSUMS in front beside the two #defines of the terms form, and the same evaluation code is compiled for that many sums.
//
// The quadratic form (pchip_source_create_quad): a Gaussian in data space with a dense precision matrix.  The source defines pchip_residual
// (the i-th residual, one lane per i) and pchip_logl_finish (the terms form's own, of the finished chi2 = r^T P r); the matrix is copied
// with the data and lies BEHIND the user's data in the handle's block (the form's ntail doubles: a run uploads both in one piece, the
// user's functions see data / ndata as given).  Such a handle is a terms handle of nres terms and one sum to everybody who asks, and its
// unit gets PCHIP_USER_QUAD in front beside the two #defines of the terms form: pc_sample.hip's walk over the matrix is compiled in
// their place only.
//
// The BATCHED quadratic form (pchip_source_create_quad_batch): the same two functions and the same block (the matrix behind the data), up to
// PCHIP_SOURCE_MAX_RES_BATCH residuals, and NO in-kernel evaluation: a round's parked proposals are evaluated together, three launches a
// tick, chi2 on the matrix cores (pc_quad_mm.hip).  Its form has nterms == nquad == 0 and nbatch = nres; its unit gets PCHIP_USER_QUAD_BATCH and
// PCHIP_SRC_NRES in front, under which pc_sample.hip compiles k_quad_residuals and k_quad_finish -- the only kernels its module is asked for.
//
// Shared values (pchip_source_create_shared): the source defines pchip_shared_value (the k-th of nshared values of theta that do not depend
// on i, one lane per k, once per evaluated point) and the functions of its form -- terms, sums or quadratic -- as overloads with `const
// double *shared` behind theta.  Such a handle is what its form is to everybody who asks, and its unit gets PCHIP_USER_SHARED and
// PCHIP_SRC_NSHARED in front beside the form's own #defines.
//
// A prior in the same source (pchip_source_create_prior): the text defines pchip_prior_param (theta[i] from the whole cube, one call per
// parameter) next to the likelihood of either form; such a handle's unit gets PCHIP_USER_PRIOR in front, and a run with prior.kind =
// PCHIP_PRIOR_SOURCE takes the table's kernel variants with that function behind the transform's one entry point (pc_sample.hip).
//
// What a handle is stands in ONE record, its PcSourceForm (pc_launch.h): the seven pchip_source_create* doors fill it through one creation
// path (pc_rtc_source_create; one ladder of refusals, spec_refusal), the unit of the kernels and the probe unit of the quick compile are
// generated from it, and everybody else -- the launchers for their LDS, the engine, the doors -- reads it with pc_rtc_source_form, once.
// pchip_source_destroy releases the text and the data and leaves the form, alive = 0: launch shapes stay right for a run in flight, and
// whatever starts work (a run's set-up, the eval entry points, a compilation) refuses the handle as one that does not exist.  The data
// block is handed out as a hold (pc_rtc_source_hold), never as a bare pointer into the registry.
//
// settings.ablate bit 15 sends the built-in kinds the same way (a module without a user source): the test that
// this path is the static kernel.
//
// libhiprtc is opened with dlopen: without it the library loads and the built-ins run; a source run then fails with a message.
#include "pc_state.h"
#include "pc_launch.h"
#include "../../include/polychord_hip.h"
#include <hip/hiprtc.h>          // types only: the library is dlopen'ed
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <tuple>
#include <chrono>
#include <vector>

#include "pc_rtc_sources.inc"    // generated (Makefile): pc_rtc_src_name[], pc_rtc_src_text[], pc_rtc_nsrc

namespace {

struct Hiprtc {
    void *h = nullptr; bool tried = false; std::string why;
    hiprtcResult (*CreateProgram)(hiprtcProgram *, const char *, const char *, int, const char **, const char **) = nullptr;
    hiprtcResult (*DestroyProgram)(hiprtcProgram *) = nullptr;
    hiprtcResult (*AddNameExpression)(hiprtcProgram, const char *) = nullptr;
    hiprtcResult (*CompileProgram)(hiprtcProgram, int, const char *const *) = nullptr;
    hiprtcResult (*GetLoweredName)(hiprtcProgram, const char *, const char **) = nullptr;
    hiprtcResult (*GetProgramLogSize)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*GetProgramLog)(hiprtcProgram, char *) = nullptr;
    hiprtcResult (*GetCodeSize)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*GetCode)(hiprtcProgram, char *) = nullptr;
    bool load()
    {   // (under the registry's compile mutex)
        if (tried) return h != nullptr;
        tried = true;
        const char *env = std::getenv("PCHIP_HIPRTC_LIB");
        const char *names[] = { env, "libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6", "/opt/rocm/lib/libhiprtc.so" };
        for (const char *n : names) {
            if (!n || !*n) continue;
            if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        }
        if (!h) { why = "libhiprtc could not be loaded (set PCHIP_HIPRTC_LIB to its path)"; return false; }
#define PC_SYM(f) f = (decltype(f))dlsym(h, "hiprtc" #f); if (!f) { why = "libhiprtc lacks hiprtc" #f; h = nullptr; return false; }
        PC_SYM(CreateProgram) PC_SYM(DestroyProgram) PC_SYM(AddNameExpression) PC_SYM(CompileProgram) PC_SYM(GetLoweredName)
        PC_SYM(GetProgramLogSize) PC_SYM(GetProgramLog) PC_SYM(GetCodeSize) PC_SYM(GetCode)
#undef PC_SYM
        return true;
    }
};

// a registered handle: never changed once it is in the registry (a compilation or an upload on another thread reads it without the lock).
// pchip_source_destroy puts a record of the form alone in its place -- alive = 0, no text, no data
struct Source {
    PcSourceForm form{};                   // what the handle is (pc_launch.h)
    std::string text;                      // the user's source, behind the #define lines of its options
    std::shared_ptr<const std::vector<double>> data;      // the user's form.ndata doubles, then form.ntail of the handle's own (pc_rtc_source_hold)
};

// a code object of one kernel variant for one architecture: compiled once, loaded on every device of that architecture
struct Code {
    std::mutex m;                          // held by the thread that compiles it; the others wait for the result
    bool done = false;
    std::vector<char> code; std::string lowered, err;
};

struct Registry {
    std::mutex m;                          // the maps below; never held across a compilation or a module load
    std::mutex cm;                         // hiprtc itself: one compilation at a time
    Hiprtc rtc;
    // every handle ever made: a destroyed one keeps its form (a few dozen bytes a handle for the life of the process, the accepted cost of
    // launch shapes that stay right for a run still in flight)
    std::map<int, std::shared_ptr<const Source>> src;
    int next = 1;
    std::map<std::tuple<int, std::string, std::string>, std::shared_ptr<Code>> code;   // (source, arch, kernel name)
    // (source, device, kernel name) -> function; modules stay loaded for the life of the process (a run may hold the function)
    std::map<std::tuple<int, int, std::string>, hipFunction_t> fn;
    std::map<int, std::string> arch;       // device -> gcnArchName
    double compile_s = 0.0; long compiles = 0;
};
Registry &reg() { static Registry *r = new Registry; return *r; }

thread_local std::string t_err;            // why the last pc_rtc_launch of this thread failed (the engine words the run's error from it)

const char *const USER_NAME = "pchip_user_source.h";

// the user's options: -DNAME[=VALUE] and -UNAME only, turned into #define / #undef lines in front of the user's text (and nowhere else:
// the library's kernels keep their own compilation).  Anything else: "" and the offending option in *bad.
std::string options_to_defines(const char *o, std::string *bad)
{
    std::string out;
    if (!o) return out;
    std::istringstream is(o);
    std::string w;
    while (is >> w) {
        if (w.size() > 2 && w.compare(0, 2, "-D") == 0) {
            const std::string d = w.substr(2);
            const size_t eq = d.find('=');
            out += "#define " + (eq == std::string::npos ? d + " 1" : d.substr(0, eq) + " " + d.substr(eq + 1)) + "\n";
        } else if (w.size() > 2 && w.compare(0, 2, "-U") == 0) out += "#undef " + w.substr(2) + "\n";
        else { *bad = w; return ""; }
    }
    return out;
}

// one hiprtc program: the user's source (as the header pchip_user_source.h, when there is one), the embedded kernel sources and `unit`;
// the names in `exprs` are instantiated and their lowered names returned.  0: ok (code filled); else the log in `log`.
int compile(const Source *s, const std::string &unit, const std::vector<std::string> &exprs, const std::string &arch,
            std::vector<char> &code, std::vector<std::string> &lowered, std::string &log)
{
    Hiprtc &R = reg().rtc;
    std::lock_guard<std::mutex> g(reg().cm);
    if (!R.load()) { log = R.why; return 1; }
    std::vector<const char *> hdr, names;
    for (int i = 0; i < pc_rtc_nsrc; ++i) { hdr.push_back(pc_rtc_src_text[i]); names.push_back(pc_rtc_src_name[i]); }
    if (s) { hdr.push_back(s->text.c_str()); names.push_back(USER_NAME); }
    hiprtcProgram p;
    if (R.CreateProgram(&p, unit.c_str(), "pchip_rtc_unit.hip", (int)hdr.size(), hdr.data(), names.data()) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed"; return 1;
    }
    for (const auto &e : exprs) R.AddNameExpression(p, e.c_str());
    // the options of the library's own kernels (Makefile CXXFLAGS: -O3 -std=c++17) and the device's architecture as reported
    const std::vector<std::string> opt = { "--offload-arch=" + arch, "-O3", "-std=c++17", "-Wno-unused-value" };
    std::vector<const char *> o;
    for (const auto &x : opt) o.push_back(x.c_str());
    const hiprtcResult rc = R.CompileProgram(p, (int)o.size(), o.data());
    size_t n = 0;
    R.GetProgramLogSize(p, &n);
    log.assign(n, '\0');
    if (n) { R.GetProgramLog(p, &log[0]); log.resize(std::strlen(log.c_str())); }
    if (rc != HIPRTC_SUCCESS) { R.DestroyProgram(&p); if (log.empty()) log = "hiprtc: compilation failed"; return 1; }
    lowered.clear();
    for (const auto &e : exprs) {
        const char *ln = nullptr;
        if (R.GetLoweredName(p, e.c_str(), &ln) != HIPRTC_SUCCESS || !ln) { R.DestroyProgram(&p); log = "hiprtc: no kernel " + e; return 1; }
        lowered.push_back(ln);
    }
    R.GetCodeSize(p, &n);
    code.resize(n);
    R.GetCode(p, code.data());
    R.DestroyProgram(&p);
    return 0;
}

// the translation unit of the sampling kernels: the library's kernels (pc_sample.hip declares pchip_loglikelihood under PCHIP_USER_SOURCE),
// then the user's text -- its macros and pragmas reach nothing of the library's.  In front, what the handle's form says: a prior in the
// source PCHIP_USER_PRIOR; the terms form PCHIP_USER_TERMS and its loop bound, and beside them the number of sums of a handle with several,
// PCHIP_USER_QUAD of a quadratic form, PCHIP_USER_SHARED and their number of a handle with shared values
std::string kernel_unit(const Source *s)
{
    if (!s) return "#include \"pc_sample.hip\"\n";
    const PcSourceForm &f = s->form;
    std::string u = f.has_prior ? "#define PCHIP_USER_PRIOR 1\n" : "";
    if (f.nbatch > 0) u += "#define PCHIP_USER_QUAD_BATCH 1\n#define PCHIP_SRC_NRES " + std::to_string(f.nbatch) + "L\n";
    if (f.nterms > 0) {
        if (f.nsums > 0) u += "#define PCHIP_USER_SUMS 1\n#define PCHIP_SRC_NSUMS " + std::to_string(f.nsums) + "\n";
        if (f.nquad > 0) u += "#define PCHIP_USER_QUAD 1\n";
        if (f.nshared > 0) u += "#define PCHIP_USER_SHARED 1\n#define PCHIP_SRC_NSHARED " + std::to_string(f.nshared) + "\n";
    }
    u += "#define PCHIP_USER_SOURCE 1\n";
    if (f.nterms > 0) u += "#define PCHIP_USER_TERMS 1\n#define PCHIP_SRC_NTERMS " + std::to_string(f.nterms) + "L\n";
    return u + "#include \"pc_sample.hip\"\n#include \"" + USER_NAME + "\"\n";
}

// The quick compile of pchip_source_create and its kin: the user's functions alone, declared with the signatures of the handle's form and
// called once each from a small kernel -- a source that lacks one fails at the link of this unit, by that function's name.  The per-item
// function of the form (pchip_logl_term, pchip_logl_terms, pchip_residual) and its finish take `const double *shared` behind theta where the
// handle has shared values: those overloads are then the only ones declared.  The user's text comes last, behind its own `#line 1`.
std::string probe_unit(const PcSourceForm &f)
{
    const std::string D = "const double *data, long ndata", SH = f.nshared > 0 ? "const double *shared, " : "", sh = f.nshared > 0 ? "sh, " : "";
    std::string decl, body;
    if (f.nshared > 0) {
        decl += "__device__ double pchip_shared_value(const double *theta, int nDims, " + D + ", long k);\n";
        body += "double sh[2]; sh[0] = pchip_shared_value(th, nDims, data, ndata, i); ";
    }
    if (f.nbatch > 0) {                          // (the batched quadratic form: the quadratic form's two functions, never with shared values)
        decl += "__device__ double pchip_residual(const double *theta, int nDims, " + D + ", long i);\n"
                "__device__ double pchip_logl_finish(double chi2, const double *theta, double *phi, int nDims, int nDerived, " + D + ");\n";
        body += "out[0] = pchip_logl_finish(pchip_residual(th, nDims, data, ndata, i), th, phi, nDims, nDerived, data, ndata);";
    } else if (f.nterms <= 0) {
        decl += "__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, " + D + ");\n";
        body += "out[0] = pchip_loglikelihood(th, phi, nDims, nDerived, data, ndata);";
    } else if (f.nsums > 0) {
        decl += "#define PCHIP_SRC_NSUMS " + std::to_string(f.nsums) + "\n"
                "__device__ void pchip_logl_terms(const double *theta, " + SH + "int nDims, " + D + ", long i, double *t);\n"
                "__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, " + SH + "double *phi, int nDims, int nDerived, " + D + ");\n";
        body += "double t[PCHIP_SRC_NSUMS]; pchip_logl_terms(th, " + sh + "nDims, data, ndata, i, t); "
                "out[0] = pchip_logl_finish_sums(t, th, " + sh + "phi, nDims, nDerived, data, ndata);";
    } else {
        const std::string item = f.nquad > 0 ? "pchip_residual" : "pchip_logl_term";
        decl += "__device__ double " + item + "(const double *theta, " + SH + "int nDims, " + D + ", long i);\n"
                "__device__ double pchip_logl_finish(double " + (f.nquad > 0 ? "chi2" : "sum") + ", const double *theta, " + SH + "double *phi, int nDims, int nDerived, " + D + ");\n";
        body += "out[0] = pchip_logl_finish(" + item + "(th, " + sh + "nDims, data, ndata, i), th, " + sh + "phi, nDims, nDerived, data, ndata);";
    }
    if (f.has_prior) {
        decl += "__device__ double pchip_prior_param(const double *cube, int i, int nDims, " + D + ");\n";
        body += " out[0] += pchip_prior_param(th, 0, nDims, data, ndata);";
    }
    return decl + "__global__ void pchip_probe(const double *th, double *phi, int nDims, int nDerived, " + D + ", long i, double *out)\n{ " + body + " }\n"
           "#include \"" + USER_NAME + "\"\n";
}

std::string strip_parens(const char *expr)
{
    std::string e(expr);
    while (e.size() >= 2 && e.front() == '(' && e.back() == ')') e = e.substr(1, e.size() - 2);
    return e;
}

// the live handle `id` (under the registry's lock), or nullptr: never made, or destroyed -- what everything that starts work asks
std::shared_ptr<const Source> live_source(Registry &G, int id)
{
    auto it = G.src.find(id);
    return it != G.src.end() && it->second->form.alive ? it->second : nullptr;
}
std::string no_handle(int id) { return "device source handle " + std::to_string(id) + " does not exist"; }

hipFunction_t get_function(int id, const std::string &expr, std::string &err)
{
    Registry &G = reg();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { err = "no HIP device"; return nullptr; }
    const auto key = std::make_tuple(id, dev, expr);
    std::shared_ptr<const Source> s;
    std::string arch;
    {
        std::lock_guard<std::mutex> g(G.m);
        auto it = G.fn.find(key);
        if (it != G.fn.end()) return it->second;      // (a destroyed handle's too: a run in flight goes on with what it has)
        if (id != 0 && !(s = live_source(G, id))) { err = no_handle(id); return nullptr; }
        auto ai = G.arch.find(dev);
        if (ai == G.arch.end()) {
            hipDeviceProp_t pr;
            if (hipGetDeviceProperties(&pr, dev) != hipSuccess) { err = "hipGetDeviceProperties failed"; return nullptr; }
            ai = G.arch.emplace(dev, std::string(pr.gcnArchName)).first;
        }
        arch = ai->second;
    }
    std::shared_ptr<Code> c;
    {
        std::lock_guard<std::mutex> g(G.m);
        auto &slot = G.code[std::make_tuple(id, arch, expr)];
        if (!slot) slot = std::make_shared<Code>();
        c = slot;
    }
    {
        std::lock_guard<std::mutex> g(c->m);      // (the first thread compiles; others asking for the same code wait here, nobody else does)
        if (!c->done) {
            std::vector<std::string> lowered; std::string log;
            const auto t0 = std::chrono::steady_clock::now();
            if (compile(s.get(), kernel_unit(s.get()), { expr }, arch, c->code, lowered, log)) c->err = "run-time compilation of " + expr + " failed:\n" + log;
            else c->lowered = lowered[0];
            c->done = true;
            std::lock_guard<std::mutex> g2(G.m);
            G.compile_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); G.compiles++;
        }
    }
    if (!c->err.empty()) { err = c->err; return nullptr; }
    hipModule_t mod;
    if (hipModuleLoadData(&mod, c->code.data()) != hipSuccess) { (void)hipGetLastError(); err = "hipModuleLoadData failed for " + expr; return nullptr; }
    hipFunction_t f;
    if (hipModuleGetFunction(&f, mod, c->lowered.c_str()) != hipSuccess) { (void)hipGetLastError(); err = "hipModuleGetFunction failed for " + expr; return nullptr; }
    std::lock_guard<std::mutex> g(G.m);
    auto ins = G.fn.emplace(key, f);
    if (!ins.second) (void)hipModuleUnload(mod);   // another thread of this device loaded it meanwhile: keep one
    return ins.first->second;
}

}  // namespace

extern "C" {

// launched by PC_LAUNCH (pc_sample.hip) with the variant, grid, block, dynamic LDS and arguments the launcher chose for the static kernel
int pc_rtc_launch(const PcState *S, const char *expr, dim3 grid, dim3 block, size_t sh, hipStream_t st, void **args)
{
    t_err.clear();
    const std::string e = strip_parens(expr);
    hipFunction_t f = get_function(S->like.kind == PC_LIKE_SOURCE ? S->src_id : 0, e, t_err);
    if (!f) return 1;
    // (module functions have no dynamic-LDS attribute to raise: the launch is checked against the device's limit per workgroup)
    int dev = 0, lim = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && sh > (size_t)lim) {
        t_err = e + ": " + std::to_string(sh) + " bytes of LDS, the device has " + std::to_string(lim); return 1;
    }
    if (hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)sh, st, args, nullptr) != hipSuccess) {
        t_err = std::string("hipModuleLaunchKernel failed for ") + e + ": " + hipGetErrorString(hipGetLastError()); return 1;
    }
    return 0;
}
const char *pc_rtc_error(void) { return t_err.empty() ? nullptr : t_err.c_str(); }

// the form of handle `id` in *f (zeroed first): one lock, one lookup.  0, or non-zero for an id that never existed; a destroyed handle
// answers what it answered alive, with alive = 0
int pc_rtc_source_form(int id, PcSourceForm *f)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    *f = it == G.src.end() ? PcSourceForm{} : it->second->form;
    return it == G.src.end();
}

}  // extern "C"

// a hold on the data block of a live handle (pc_launch.h), or nullptr: no such handle, or destroyed
std::shared_ptr<const std::vector<double>> pc_rtc_source_hold(int id, PcSourceForm *f)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    const std::shared_ptr<const Source> s = live_source(G, id);
    if (s && f) *f = s->form;
    return s ? s->data : nullptr;
}

// ---- C engine API ---------------------------------------------------------------------------------------------------------------------
namespace {

// what one of the seven pchip_source_create* doors was asked for: the door, the text, the data, and the fields of the form it takes
struct PcSourceSpec {
    enum Door { PLAIN, TERMS, PRIOR, SUMS, QUAD, SHARED, QUAD_BATCH } door;
    const char *source, *options; const double *data; long ndata;
    long nterms = 0; int nsums = 0; long nres = 0; const double *precision = nullptr; long nshared = 0; bool prior = false;
};

// why a spec is refused, in its door's name and words ("": it is not) -- every refusal before any device call; *defs: the options as #define lines
std::string spec_refusal(const PcSourceSpec &c, std::string *defs)
{
    static const char *const names[] = { "pchip_source_create", "pchip_source_create_terms", "pchip_source_create_prior", "pchip_source_create_sums",
                                         "pchip_source_create_quad", "pchip_source_create_shared", "pchip_source_create_quad_batch" };
    const std::string me = std::string(names[c.door]) + ": ";
    auto says = [&](const char *field, long v, const std::string &rule) { return me + field + " = " + std::to_string(v) + " -- " + rule; };
    const std::string sums_range = "1 <= nsums <= " + std::to_string(PCHIP_SOURCE_MAX_SUMS) + " (PCHIP_SOURCE_MAX_SUMS)";
    const std::string res_range = "1 <= nres <= " + std::to_string(PCHIP_SOURCE_MAX_RES) + " (PCHIP_SOURCE_MAX_RES)";
    const std::string no_matrix = me + "precision == NULL -- the nres x nres matrix of the quadratic form (host, row-major)";
    const int d = c.door;
    if (d == PcSourceSpec::TERMS && c.nterms < 1) return says("nterms", c.nterms, "the sum needs at least one term (nterms >= 1)");
    if (d == PcSourceSpec::PRIOR && c.nterms < 0) return says("nterms", c.nterms, "0 (the plain form) or the number of terms (nterms >= 1)");
    if (d == PcSourceSpec::SUMS && c.nterms < 1) return says("nterms", c.nterms, "the sums need at least one term (nterms >= 1)");
    if (d == PcSourceSpec::SUMS && (c.nsums < 1 || c.nsums > PCHIP_SOURCE_MAX_SUMS)) return says("nsums", c.nsums, sums_range);
    if (d == PcSourceSpec::QUAD && (c.nres < 1 || c.nres > PCHIP_SOURCE_MAX_RES)) return says("nres", c.nres, res_range);
    if (d == PcSourceSpec::QUAD && !c.precision) return no_matrix;
    if (d == PcSourceSpec::QUAD_BATCH && (c.nres < 1 || c.nres > PCHIP_SOURCE_MAX_RES_BATCH))
        return says("nres", c.nres, "1 <= nres <= " + std::to_string(PCHIP_SOURCE_MAX_RES_BATCH) + " (PCHIP_SOURCE_MAX_RES_BATCH)");
    if (d == PcSourceSpec::QUAD_BATCH && !c.precision) return no_matrix;
    if (d == PcSourceSpec::SHARED) {      // beside one of the three wave-parallel forms: nres > 0 the quadratic form, else nterms >= 1 terms in one sum (nsums == 0) or in nsums
        if (c.nshared < 1 || c.nshared > PCHIP_SOURCE_MAX_SHARED)
            return says("nshared", c.nshared, "1 <= nshared <= " + std::to_string(PCHIP_SOURCE_MAX_SHARED) + " (PCHIP_SOURCE_MAX_SHARED)");
        if (c.nres < 0 || c.nres > PCHIP_SOURCE_MAX_RES) return says("nres", c.nres, "0, or the quadratic form with " + res_range);
        if (c.nres > 0 && (c.nterms != 0 || c.nsums != 0))
            return me + "nres = " + std::to_string(c.nres) + " with nterms = " + std::to_string(c.nterms) + ", nsums = " + std::to_string(c.nsums) +
                   " -- one form a handle: the quadratic form (nres > 0) takes nterms == 0 and nsums == 0";
        if (c.nres > 0 && !c.precision) return no_matrix;
        if (c.nres == 0 && c.precision) return me + "precision != NULL with nres = 0 -- the matrix belongs to the quadratic form (nres > 0)";
        if (c.nres == 0 && c.nterms < 1) return says("nterms", c.nterms, "the sum needs at least one term (nterms >= 1; a plain likelihood with shared values is nterms = 1)");
        if (c.nres == 0 && (c.nsums < 0 || c.nsums > PCHIP_SOURCE_MAX_SUMS)) return says("nsums", c.nsums, "0 (one sum), or " + sums_range);
    }
    // what every door asks, in the first one's name
    if (!c.source) return "pchip_source_create: no source";
    if (c.ndata < 0 || (c.ndata > 0 && !c.data)) return "pchip_source_create: ndata > 0 needs a data block";
    std::string bad;
    *defs = options_to_defines(c.options, &bad);
    if (!bad.empty()) return "pchip_source_create: option " + bad + " -- only -DNAME[=VALUE] and -UNAME are passed on";
    return "";
}

// pchip_source_create[_terms | _prior | _sums | _quad | _shared | _quad_batch]: checks the spec, compiles the user's functions alone (a syntax error surfaces
// here, with the compiler's log) and registers the handle.  A quadratic form (nres > 0) is a terms handle of nres terms whose matrix is copied
// behind the data; the batched quadratic form keeps the matrix in the same place and is no terms handle.  Returns the handle (> 0), or -1 with the reason behind pchip_last_error.
int pc_rtc_source_create(const PcSourceSpec &c)
{
    std::string defs, log = spec_refusal(c, &defs);
    int id = -1;
    if (log.empty()) {
        auto s = std::make_shared<Source>();
        PcSourceForm &f = s->form;
        const bool batched = c.door == PcSourceSpec::QUAD_BATCH;
        f.nterms = batched ? 0 : (c.nres > 0 ? c.nres : c.nterms); f.nsums = c.nsums; f.nquad = batched ? 0 : c.nres; f.nshared = c.nshared; f.has_prior = c.prior;
        f.nbatch = batched ? (int)c.nres : 0;
        f.ndata = c.ndata; f.ntail = (long long)c.nres * c.nres; f.alive = 1;
        s->text = defs + "#line 1\n" + c.source;
        std::vector<double> block;
        if (c.ndata > 0) block.assign(c.data, c.data + c.ndata);
        block.insert(block.end(), c.precision, c.precision + f.ntail);
        s->data = std::make_shared<const std::vector<double>>(std::move(block));
        std::string arch = "gfx950";
        int dev = 0, ndev = 0;
        if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipGetDevice(&dev) == hipSuccess) {
            hipDeviceProp_t pr;
            if (hipGetDeviceProperties(&pr, dev) == hipSuccess) arch = pr.gcnArchName;
        }
        (void)hipGetLastError();
        std::vector<char> code; std::vector<std::string> lowered;
        if (!compile(s.get(), probe_unit(f), { "pchip_probe" }, arch, code, lowered, log)) {
            Registry &G = reg();
            std::lock_guard<std::mutex> g(G.m);
            id = G.next++; G.src[id] = s;
        }
    }
    pc_abi_set_last_error(id > 0 ? nullptr : log.c_str());
    return id;
}

}  // namespace

// the seven doors (the spec's fields in order: door, source, options, data, ndata, nterms, nsums, nres, precision, nshared, prior).  _prior:
// nterms == 0 the plain form of likelihood, nterms >= 1 the terms form; with_prior: pchip_prior_param in the same source
extern "C" int pchip_source_create(const char *source, const char *options, const double *data, long ndata) { return pc_rtc_source_create({ PcSourceSpec::PLAIN, source, options, data, ndata }); }
extern "C" int pchip_source_create_terms(const char *source, const char *options, const double *data, long ndata, long nterms) { return pc_rtc_source_create({ PcSourceSpec::TERMS, source, options, data, ndata, nterms }); }
extern "C" int pchip_source_create_prior(const char *source, const char *options, const double *data, long ndata, long nterms)
{
    return pc_rtc_source_create({ PcSourceSpec::PRIOR, source, options, data, ndata, nterms, 0, 0, nullptr, 0, true });
}
extern "C" int pchip_source_create_sums(const char *source, const char *options, const double *data, long ndata, long nterms, int nsums, int with_prior)
{
    return pc_rtc_source_create({ PcSourceSpec::SUMS, source, options, data, ndata, nterms, nsums, 0, nullptr, 0, with_prior != 0 });
}
extern "C" int pchip_source_create_quad(const char *source, const char *options, const double *data, long ndata, long nres, const double *precision,
                                        int with_prior)
{
    return pc_rtc_source_create({ PcSourceSpec::QUAD, source, options, data, ndata, 0, 0, nres, precision, 0, with_prior != 0 });
}
extern "C" int pchip_source_create_quad_batch(const char *source, const char *options, const double *data, long ndata, long nres, const double *precision)
{
    return pc_rtc_source_create({ PcSourceSpec::QUAD_BATCH, source, options, data, ndata, 0, 0, nres, precision, 0, false });
}
extern "C" int pchip_source_create_shared(const char *source, const char *options, const double *data, long ndata, long nshared, long nterms, int nsums,
                                          long nres, const double *precision, int with_prior)
{
    return pc_rtc_source_create({ PcSourceSpec::SHARED, source, options, data, ndata, nterms, nsums, nres, precision, nshared, with_prior != 0 });
}

// The text and the data go -- a hold taken before (pc_rtc_source_hold) keeps the block for as long as somebody copies from it --, the form
// stays, alive = 0: a run on another thread may still launch the handle's compiled modules, which stay loaded, and its launchers size their
// LDS from the form on every launch.  The price is the form's few dozen bytes for every handle ever made.
extern "C" void pchip_source_destroy(int handle)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(handle);
    if (it == G.src.end() || !it->second->form.alive) return;
    auto dead = std::make_shared<Source>();
    dead->form = it->second->form; dead->form.alive = 0;
    it->second = dead;
}

// the embedded text of kernel source `i` (its file name in *name), or NULL past the last: tests compare it with the files
extern "C" const char *pchip_rtc_embedded_source(int i, const char **name)
{
    if (i < 0 || i >= pc_rtc_nsrc) return nullptr;
    if (name) *name = pc_rtc_src_name[i];
    return pc_rtc_src_text[i];
}

// compiles, for architecture `arch`, the sampling kernels named in `names` (';'-separated name expressions) with source `handle` (0: the
// built-ins alone) -- what a run on such a device would compile, without a device.  0: ok; else the log in log[cap].
extern "C" int pchip_rtc_compile_check(int handle, const char *arch, const char *names, char *log, int cap, double *seconds)
{
    std::shared_ptr<const Source> s;
    {
        Registry &G = reg();
        std::lock_guard<std::mutex> g(G.m);
        if (handle && !(s = live_source(G, handle))) { if (log && cap > 0) std::snprintf(log, cap, "%s", no_handle(handle).c_str()); return 1; }
    }
    std::vector<std::string> exprs;
    std::string all(names ? names : ""), e;
    std::istringstream is(all);
    while (std::getline(is, e, ';')) if (!e.empty()) exprs.push_back(e);
    std::vector<char> code; std::vector<std::string> lowered; std::string lg;
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    rc = compile(s.get(), kernel_unit(s.get()), exprs, arch ? arch : "gfx950", code, lowered, lg);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (log && cap > 0) std::snprintf(log, cap, "%s", rc ? lg.c_str() : "");
    return rc ? 1 : (code.empty() ? 1 : 0);
}

// run-time compilations so far and the seconds they took (measurement)
extern "C" void pchip_rtc_stats(long *compiles, double *seconds)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    if (compiles) *compiles = G.compiles;
    if (seconds) *seconds = G.compile_s;
}
