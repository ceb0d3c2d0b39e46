// pc_rtc.hip -- user likelihoods written as HIP device source, fused into the sampling kernels at run time.
//
// A source (pchip_source_create) is a string that defines
//     __device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);
// The library compiles it with hiprtc, together with the exact text of its own sampling kernels (pc_dev.h, pc_state.h, pc_sample.hip and
// the bodies it includes, embedded when the library is built: pc_rtc_sources.inc), for the device a run is on.  The launchers of
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
// with the data and lies BEHIND the user's data in the handle's block (pc_rtc_source_tail doubles: a run uploads both in one piece, the
// user's functions see data / ndata as given).  Such a handle is a terms handle of nres terms and one sum to everybody who asks, and its
// unit gets PCHIP_USER_QUAD in front beside the two #defines of the terms form: pc_sample.hip's walk over the matrix is compiled in
// their place only.
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

struct Source {
    std::string text;                      // the user's source, behind the #define lines of its options
    std::vector<double> data;
    long nterms = 0;                       // > 0: the terms form (pchip_logl_term / pchip_logl_finish), the sum's length
    int nsums = 0;                         // > 0: several sums per evaluation (pchip_logl_terms / pchip_logl_finish_sums; pchip_source_create_sums)
    long nquad = 0;                        // > 0: the quadratic form (pchip_residual / pchip_logl_finish; pchip_source_create_quad): nterms == nquad, and
                                           //      the nquad x nquad precision matrix lies in `data` behind the user's ndata doubles
    long nshared = 0;                      // > 0: shared values (pchip_shared_value; pchip_source_create_shared) beside the form above
    long long ndata = 0;                   // the user's data: the first ndata doubles of `data`
    bool has_prior = false;                // the source defines pchip_prior_param as well (pchip_source_create_prior)
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
    std::map<int, std::shared_ptr<Source>> src;
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
// then the user's text -- its macros and pragmas reach nothing of the library's.  A terms handle: its form and its loop bound in front;
// a handle with several sums: their number in front as well; a quadratic form: PCHIP_USER_QUAD in front as well; shared values: PCHIP_USER_SHARED and their number in front as well; a handle with a prior (pchip_source_create_prior): PCHIP_USER_PRIOR in front.
std::string kernel_unit(const Source *s)
{
    const std::string prior = s && s->has_prior ? "#define PCHIP_USER_PRIOR 1\n" : "";
    const std::string sums = s && s->nsums > 0 ? "#define PCHIP_USER_SUMS 1\n#define PCHIP_SRC_NSUMS " + std::to_string(s->nsums) + "\n" : "";
    const std::string quad = s && s->nquad > 0 ? "#define PCHIP_USER_QUAD 1\n" : "";
    const std::string shared = s && s->nshared > 0 ? "#define PCHIP_USER_SHARED 1\n#define PCHIP_SRC_NSHARED " + std::to_string(s->nshared) + "\n" : "";
    if (s && s->nterms > 0)
        return prior + sums + quad + shared + "#define PCHIP_USER_SOURCE 1\n#define PCHIP_USER_TERMS 1\n#define PCHIP_SRC_NTERMS " + std::to_string(s->nterms) + "L\n#include \"pc_sample.hip\"\n#include \"" + USER_NAME + "\"\n";
    return s ? prior + "#define PCHIP_USER_SOURCE 1\n#include \"pc_sample.hip\"\n#include \"" + USER_NAME + "\"\n"
             : std::string("#include \"pc_sample.hip\"\n");
}

// the quick compile of pchip_source_create: the user's functions alone behind the same declaration, called from a small kernel
const char *const PROBE_UNIT =
    "__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);\n"
    "__global__ void pchip_probe(const double *th, double *phi, int nDims, int nDerived, const double *data, long ndata, double *out)\n"
    "{ out[0] = pchip_loglikelihood(th, phi, nDims, nDerived, data, ndata); }\n"
    "#include \"pchip_user_source.h\"\n";
// ... and of pchip_source_create_terms: both functions of the terms form (a source that lacks one fails at the link of this unit, by name)
const char *const PROBE_UNIT_TERMS =
    "__device__ double pchip_logl_term(const double *theta, int nDims, const double *data, long ndata, long i);\n"
    "__device__ double pchip_logl_finish(double sum, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);\n"
    "__global__ void pchip_probe(const double *th, double *phi, int nDims, int nDerived, const double *data, long ndata, long i, double *out)\n"
    "{ out[0] = pchip_logl_finish(pchip_logl_term(th, nDims, data, ndata, i), th, phi, nDims, nDerived, data, ndata); }\n"
    "#include \"pchip_user_source.h\"\n";
// ... and of pchip_source_create_sums (behind a #define of PCHIP_SRC_NSUMS): one call of the terms, the finish of what it wrote
const char *const PROBE_UNIT_SUMS =
    "__device__ void pchip_logl_terms(const double *theta, int nDims, const double *data, long ndata, long i, double *t);\n"
    "__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);\n"
    "__global__ void pchip_probe(const double *th, double *phi, int nDims, int nDerived, const double *data, long ndata, long i, double *out)\n"
    "{ double t[PCHIP_SRC_NSUMS]; pchip_logl_terms(th, nDims, data, ndata, i, t); out[0] = pchip_logl_finish_sums(t, th, phi, nDims, nDerived, data, ndata); }\n"
    "#include \"pchip_user_source.h\"\n";
// ... and of pchip_source_create_quad: one residual, the finish of it
const char *const PROBE_UNIT_QUAD =
    "__device__ double pchip_residual(const double *theta, int nDims, const double *data, long ndata, long i);\n"
    "__device__ double pchip_logl_finish(double chi2, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);\n"
    "__global__ void pchip_probe(const double *th, double *phi, int nDims, int nDerived, const double *data, long ndata, long i, double *out)\n"
    "{ out[0] = pchip_logl_finish(pchip_residual(th, nDims, data, ndata, i), th, phi, nDims, nDerived, data, ndata); }\n"
    "#include \"pchip_user_source.h\"\n";
// ... and of pchip_source_create_shared: the probe of the handle's form with one shared value computed and the block passed on -- the
// overloads with `shared` behind theta are the only ones declared, so a source that has only the others fails at the link, by name
const char *const PROBE_SHARED_DECL =
    "__device__ double pchip_shared_value(const double *theta, int nDims, const double *data, long ndata, long k);\n";
const char *const PROBE_SHARED_HEAD =
    "__global__ void pchip_probe(const double *th, double *phi, int nDims, int nDerived, const double *data, long ndata, long i, double *out)\n"
    "{ double sh[2]; sh[0] = pchip_shared_value(th, nDims, data, ndata, i); ";
const char *const PROBE_UNIT_TERMS_SHARED =
    "__device__ double pchip_logl_term(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i);\n"
    "__device__ double pchip_logl_finish(double sum, const double *theta, const double *shared, double *phi, int nDims, int nDerived, const double *data, long ndata);\n"
    "%HEAD%out[0] = pchip_logl_finish(pchip_logl_term(th, sh, nDims, data, ndata, i), th, sh, phi, nDims, nDerived, data, ndata); }\n"
    "#include \"pchip_user_source.h\"\n";
const char *const PROBE_UNIT_SUMS_SHARED =
    "__device__ void pchip_logl_terms(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i, double *t);\n"
    "__device__ double pchip_logl_finish_sums(const double *sums, const double *theta, const double *shared, double *phi, int nDims, int nDerived, const double *data, long ndata);\n"
    "%HEAD%double t[PCHIP_SRC_NSUMS]; pchip_logl_terms(th, sh, nDims, data, ndata, i, t); out[0] = pchip_logl_finish_sums(t, th, sh, phi, nDims, nDerived, data, ndata); }\n"
    "#include \"pchip_user_source.h\"\n";
const char *const PROBE_UNIT_QUAD_SHARED =
    "__device__ double pchip_residual(const double *theta, const double *shared, int nDims, const double *data, long ndata, long i);\n"
    "__device__ double pchip_logl_finish(double chi2, const double *theta, const double *shared, double *phi, int nDims, int nDerived, const double *data, long ndata);\n"
    "%HEAD%out[0] = pchip_logl_finish(pchip_residual(th, sh, nDims, data, ndata, i), th, sh, phi, nDims, nDerived, data, ndata); }\n"
    "#include \"pchip_user_source.h\"\n";
std::string probe_unit_shared(int nsums, bool quad)
{
    std::string u = quad ? PROBE_UNIT_QUAD_SHARED : (nsums > 0 ? PROBE_UNIT_SUMS_SHARED : PROBE_UNIT_TERMS_SHARED);
    u.replace(u.find("%HEAD%"), 6, PROBE_SHARED_HEAD);
    return (nsums > 0 ? "#define PCHIP_SRC_NSUMS " + std::to_string(nsums) + "\n" : std::string()) + PROBE_SHARED_DECL + u;
}

// ... and of pchip_source_create_prior: the probe of the handle's form, then pchip_prior_param behind its declaration, called as well
const char *const PROBE_PRIOR_DECL =
    "__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata);\n";
const char *const PROBE_PRIOR_CALL = "out[0] += pchip_prior_param(th, 0, nDims, data, ndata); }\n";
std::string probe_unit(long nterms, int nsums, bool quad, bool prior, bool shared)
{
    std::string u = shared ? probe_unit_shared(nsums, quad) : quad ? std::string(PROBE_UNIT_QUAD) : nsums > 0 ? "#define PCHIP_SRC_NSUMS " + std::to_string(nsums) + "\n" + PROBE_UNIT_SUMS : std::string(nterms > 0 ? PROBE_UNIT_TERMS : PROBE_UNIT);
    if (!prior) return u;
    const size_t close = u.rfind(" }\n");        // the end of pchip_probe's body: the call goes in front of it
    u.replace(close, 3, std::string(" ") + PROBE_PRIOR_CALL);
    return PROBE_PRIOR_DECL + u;
}

std::string strip_parens(const char *expr)
{
    std::string e(expr);
    while (e.size() >= 2 && e.front() == '(' && e.back() == ')') e = e.substr(1, e.size() - 2);
    return e;
}

hipFunction_t get_function(int id, const std::string &expr, std::string &err)
{
    Registry &G = reg();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { err = "no HIP device"; return nullptr; }
    const auto key = std::make_tuple(id, dev, expr);
    std::shared_ptr<Source> s;
    std::string arch;
    {
        std::lock_guard<std::mutex> g(G.m);
        auto it = G.fn.find(key);
        if (it != G.fn.end()) return it->second;
        if (id != 0) {
            auto si = G.src.find(id);
            if (si == G.src.end()) { err = "device source handle " + std::to_string(id) + " does not exist"; return nullptr; }
            s = si->second;
        }
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

// a source exists (and its data block, for the engine's upload: *n of the user's doubles, pc_rtc_source_tail(id) of the handle's own behind them)
int pc_rtc_source_data(int id, const double **data, long long *n)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    if (it == G.src.end()) return 1;
    *data = it->second->data.empty() ? nullptr : it->second->data.data();
    *n = it->second->ndata;
    return 0;
}

// the doubles a handle keeps in its block BEHIND the user's data (a quadratic form: its precision matrix, nres x nres); 0: none, or no such handle
long long pc_rtc_source_tail(int id)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    return it == G.src.end() ? 0 : (long long)it->second->data.size() - it->second->ndata;
}

// the number of terms of a terms-form handle; 0: the plain form, or no such handle
long pc_rtc_source_terms(int id)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    return it == G.src.end() ? 0 : it->second->nterms;
}

// the number of sums of a handle made by pchip_source_create_sums; 0: any other handle, or none
int pc_rtc_source_sums(int id)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    return it == G.src.end() ? 0 : it->second->nsums;
}

// the number of residuals of a handle made by pchip_source_create_quad; 0: any other handle, or none
long pc_rtc_source_quad(int id)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    return it == G.src.end() ? 0 : it->second->nquad;
}

// the number of shared values of a handle made by pchip_source_create_shared; 0: any other handle, or none
long pc_rtc_source_shared(int id)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    return it == G.src.end() ? 0 : it->second->nshared;
}

int pc_rtc_source_has_prior(int id)
{
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    auto it = G.src.find(id);
    return it != G.src.end() && it->second->has_prior ? 1 : 0;
}

// pchip_source_create[_terms | _sums | _quad | _prior | _shared]: registers the source and compiles the user's functions alone (a syntax error surfaces here, with the log).
// nterms > 0: the terms form, of nsums sums where nsums > 0; precision != NULL: the quadratic form of nterms residuals, its matrix copied
// behind the data; nshared > 0: shared values beside that form.  Returns the handle (> 0), or -1 with the compiler's log in `log`.
int pc_rtc_source_create(const char *source, const char *options, const double *data, long ndata, long nterms, int nsums, bool prior, std::string *log,
                         const double *precision, long nshared = 0)
{
    if (!source) { *log = "pchip_source_create: no source"; return -1; }
    if (ndata < 0 || (ndata > 0 && !data)) { *log = "pchip_source_create: ndata > 0 needs a data block"; return -1; }
    std::string bad;
    const std::string defs = options_to_defines(options, &bad);
    if (!bad.empty()) { *log = "pchip_source_create: option " + bad + " -- only -DNAME[=VALUE] and -UNAME are passed on"; return -1; }
    auto s = std::make_shared<Source>();
    s->text = defs + "#line 1\n" + source;
    if (ndata > 0) s->data.assign(data, data + ndata);
    s->ndata = ndata;
    if (precision) { s->data.insert(s->data.end(), precision, precision + (size_t)nterms * (size_t)nterms); s->nquad = nterms; }
    s->nterms = nterms; s->nsums = nsums; s->has_prior = prior; s->nshared = nshared;
    std::string arch = "gfx950";
    int dev = 0, ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipGetDevice(&dev) == hipSuccess) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, dev) == hipSuccess) arch = pr.gcnArchName;
    }
    (void)hipGetLastError();
    std::vector<char> code; std::vector<std::string> lowered;
    if (compile(s.get(), probe_unit(nterms, nsums, precision != nullptr, prior, nshared > 0), { "pchip_probe" }, arch, code, lowered, *log)) return -1;
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    const int id = G.next++;
    G.src[id] = s;
    return id;
}

}  // extern "C"

// ---- C engine API ---------------------------------------------------------------------------------------------------------------------

extern "C" int pchip_source_create(const char *source, const char *options, const double *data, long ndata)
{
    std::string log;
    const int id = pc_rtc_source_create(source, options, data, ndata, 0, 0, false, &log, nullptr);
    pc_abi_set_last_error(id > 0 ? nullptr : log.c_str());
    return id;
}

extern "C" int pchip_source_create_terms(const char *source, const char *options, const double *data, long ndata, long nterms)
{
    std::string log;
    int id = -1;
    if (nterms < 1) log = "pchip_source_create_terms: nterms = " + std::to_string(nterms) + " -- the sum needs at least one term (nterms >= 1)";
    else id = pc_rtc_source_create(source, options, data, ndata, nterms, 0, false, &log, nullptr);
    pc_abi_set_last_error(id > 0 ? nullptr : log.c_str());
    return id;
}

// likelihood and prior in one source and one handle: nterms == 0 the plain form of likelihood, nterms >= 1 the terms form
extern "C" int pchip_source_create_prior(const char *source, const char *options, const double *data, long ndata, long nterms)
{
    std::string log;
    int id = -1;
    if (nterms < 0) log = "pchip_source_create_prior: nterms = " + std::to_string(nterms) + " -- 0 (the plain form) or the number of terms (nterms >= 1)";
    else id = pc_rtc_source_create(source, options, data, ndata, nterms, 0, true, &log, nullptr);
    pc_abi_set_last_error(id > 0 ? nullptr : log.c_str());
    return id;
}

// the terms form with nsums sums per evaluation (pchip_logl_terms / pchip_logl_finish_sums); with_prior: pchip_prior_param in the same source
extern "C" int pchip_source_create_sums(const char *source, const char *options, const double *data, long ndata, long nterms, int nsums, int with_prior)
{
    std::string log;
    int id = -1;
    if (nterms < 1) log = "pchip_source_create_sums: nterms = " + std::to_string(nterms) + " -- the sums need at least one term (nterms >= 1)";
    else if (nsums < 1 || nsums > PCHIP_SOURCE_MAX_SUMS)
        log = "pchip_source_create_sums: nsums = " + std::to_string(nsums) + " -- 1 <= nsums <= " + std::to_string(PCHIP_SOURCE_MAX_SUMS) + " (PCHIP_SOURCE_MAX_SUMS)";
    else id = pc_rtc_source_create(source, options, data, ndata, nterms, nsums, with_prior != 0, &log, nullptr);
    pc_abi_set_last_error(id > 0 ? nullptr : log.c_str());
    return id;
}

// the quadratic form: chi2 = r^T P r of nres residuals (pchip_residual / pchip_logl_finish), P copied here; with_prior as above
extern "C" int pchip_source_create_quad(const char *source, const char *options, const double *data, long ndata, long nres, const double *precision,
                                        int with_prior)
{
    std::string log;
    int id = -1;
    if (nres < 1 || nres > PCHIP_SOURCE_MAX_RES)
        log = "pchip_source_create_quad: nres = " + std::to_string(nres) + " -- 1 <= nres <= " + std::to_string(PCHIP_SOURCE_MAX_RES) + " (PCHIP_SOURCE_MAX_RES)";
    else if (!precision) log = "pchip_source_create_quad: precision == NULL -- the nres x nres matrix of the quadratic form (host, row-major)";
    else id = pc_rtc_source_create(source, options, data, ndata, nres, 0, with_prior != 0, &log, precision);
    pc_abi_set_last_error(id > 0 ? nullptr : log.c_str());
    return id;
}

// shared values beside one of the three wave-parallel forms: nres > 0 the quadratic form, else nterms >= 1 terms in one sum (nsums == 0) or in
// nsums sums; every refusal before any device call
extern "C" int pchip_source_create_shared(const char *source, const char *options, const double *data, long ndata, long nshared, long nterms, int nsums,
                                          long nres, const double *precision, int with_prior)
{
    const std::string me = "pchip_source_create_shared: ";
    std::string log;
    int id = -1;
    if (nshared < 1 || nshared > PCHIP_SOURCE_MAX_SHARED)
        log = me + "nshared = " + std::to_string(nshared) + " -- 1 <= nshared <= " + std::to_string(PCHIP_SOURCE_MAX_SHARED) + " (PCHIP_SOURCE_MAX_SHARED)";
    else if (nres < 0 || nres > PCHIP_SOURCE_MAX_RES)
        log = me + "nres = " + std::to_string(nres) + " -- 0, or the quadratic form with 1 <= nres <= " + std::to_string(PCHIP_SOURCE_MAX_RES) + " (PCHIP_SOURCE_MAX_RES)";
    else if (nres > 0 && (nterms != 0 || nsums != 0))
        log = me + "nres = " + std::to_string(nres) + " with nterms = " + std::to_string(nterms) + ", nsums = " + std::to_string(nsums) +
              " -- one form a handle: the quadratic form (nres > 0) takes nterms == 0 and nsums == 0";
    else if (nres > 0 && !precision) log = me + "precision == NULL -- the nres x nres matrix of the quadratic form (host, row-major)";
    else if (nres == 0 && precision) log = me + "precision != NULL with nres = 0 -- the matrix belongs to the quadratic form (nres > 0)";
    else if (nres == 0 && nterms < 1)
        log = me + "nterms = " + std::to_string(nterms) + " -- the sum needs at least one term (nterms >= 1; a plain likelihood with shared values is nterms = 1)";
    else if (nres == 0 && (nsums < 0 || nsums > PCHIP_SOURCE_MAX_SUMS))
        log = me + "nsums = " + std::to_string(nsums) + " -- 0 (one sum), or 1 <= nsums <= " + std::to_string(PCHIP_SOURCE_MAX_SUMS) + " (PCHIP_SOURCE_MAX_SUMS)";
    else id = pc_rtc_source_create(source, options, data, ndata, nres > 0 ? nres : nterms, nres > 0 ? 0 : nsums, with_prior != 0, &log, nres > 0 ? precision : nullptr, nshared);
    pc_abi_set_last_error(id > 0 ? nullptr : log.c_str());
    return id;
}

extern "C" void pchip_source_destroy(int handle)
{   // (compiled modules stay loaded: a run on another thread may still launch them)
    Registry &G = reg();
    std::lock_guard<std::mutex> g(G.m);
    G.src.erase(handle);
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
    std::shared_ptr<Source> s;
    {
        Registry &G = reg();
        std::lock_guard<std::mutex> g(G.m);
        if (handle) { auto it = G.src.find(handle); if (it == G.src.end()) { if (log && cap > 0) std::snprintf(log, cap, "no source %d", handle); return 1; } s = it->second; }
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
