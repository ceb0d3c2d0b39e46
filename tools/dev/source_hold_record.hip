// source_hold_record.hip -- a device-source handle's form outlives the handle, and a hold on its data block outlives it too: checked on the
// CPU, under the host sanitizers.
//
// Includes pc_rtc.hip (host code: the registry of handles) and walks one handle of each form through create, pc_rtc_source_form,
// pc_rtc_source_hold, pchip_source_destroy: the form is the same before and after but for alive, a hold taken before the destroy still reads
// the doubles that went in (the user's data, then a quadratic form's matrix), a hold asked for afterwards is refused, and destroying twice is
// harmless.  No device: the quick compile of the create calls is for gfx950, as without one.  Exit code 0 and a summary line, or 1 and what
// disagreed.  Built host-only with the address and undefined-behaviour sanitizers (make -C polychordlite_amd/csrc source_hold_record);
// tests/test_source_form.py runs it.
#include <hip/hip_runtime.h>
// (no device is asked for, wherever this runs: the registry's host code is what is under test)
#define hipGetDeviceCount(n) (*(n) = 0, hipErrorNoDevice)
#define hipGetLastError() hipSuccess
#include "pc_rtc.hip"

static std::string last_error;
extern "C" void pc_abi_set_last_error(const char *msg) { last_error = msg ? msg : ""; }

static const char *const PRIOR = "__device__ double pchip_prior_param(const double *c, int i, int, const double *, long) { return c[i]; }\n";
static const char *const PLAIN = "__device__ double pchip_loglikelihood(const double *t, double *, int, int, const double *d, long) { return t[0] * d[0]; }\n";
static const char *const TERMS =
    "__device__ double pchip_logl_term(const double *t, int, const double *d, long, long i) { return t[0] * d[i]; }\n"
    "__device__ double pchip_logl_finish(double s, const double *, double *, int, int, const double *, long) { return s; }\n";
static const char *const SUMS =
    "__device__ void pchip_logl_terms(const double *t, int, const double *d, long, long i, double *o) { for (int k = 0; k < PCHIP_SRC_NSUMS; ++k) o[k] = t[0] * d[i]; }\n"
    "__device__ double pchip_logl_finish_sums(const double *s, const double *, double *, int, int, const double *, long) { return s[0]; }\n";
static const char *const QUAD =
    "__device__ double pchip_residual(const double *t, int, const double *d, long, long i) { return t[0] - d[i]; }\n"
    "__device__ double pchip_logl_finish(double c, const double *, double *, int, int, const double *, long) { return -0.5 * c; }\n";
static const char *const SHARED =
    "__device__ double pchip_shared_value(const double *t, int, const double *, long, long k) { return t[0] + k; }\n"
    "__device__ double pchip_logl_term(const double *t, const double *s, int, const double *d, long, long i) { return s[0] * d[i]; }\n"
    "__device__ double pchip_logl_finish(double s, const double *, const double *, double *, int, int, const double *, long) { return s; }\n";

int main()
{
    const long nd = 7, nres = 3;
    std::vector<double> data(nd), P(nres * nres);
    for (long i = 0; i < nd; ++i) data[i] = 0.5 + i;
    for (long i = 0; i < nres * nres; ++i) P[i] = 100.0 + i;
    const std::string with_prior = std::string(PLAIN) + PRIOR;
    struct Case { const char *name; int id; PcSourceForm want; } cases[] = {
        { "plain", pchip_source_create(PLAIN, nullptr, data.data(), nd), { 0, 0, 0, 0, 0, nd, 0, 1 } },
        { "terms", pchip_source_create_terms(TERMS, nullptr, data.data(), nd, nd), { nd, 0, 0, 0, 0, nd, 0, 1 } },
        { "prior", pchip_source_create_prior(with_prior.c_str(), nullptr, data.data(), nd, 0), { 0, 0, 0, 0, 1, nd, 0, 1 } },
        { "sums", pchip_source_create_sums(SUMS, nullptr, data.data(), nd, nd, 5, 0), { nd, 5, 0, 0, 0, nd, 0, 1 } },
        { "quad", pchip_source_create_quad(QUAD, nullptr, data.data(), nd, nres, P.data(), 0), { nres, 0, nres, 0, 0, nd, nres * nres, 1 } },
        { "shared", pchip_source_create_shared(SHARED, nullptr, data.data(), nd, 4, nd, 0, 0, nullptr, 0), { nd, 0, 0, 4, 0, nd, 0, 1 } },
    };
    int bad = 0;
    auto fail = [&](const char *name, const std::string &what) { std::fprintf(stderr, "%s: %s\n", name, what.c_str()); ++bad; };
    auto same = [](const PcSourceForm &a, const PcSourceForm &b) {
        return a.nterms == b.nterms && a.nsums == b.nsums && a.nquad == b.nquad && a.nshared == b.nshared && a.has_prior == b.has_prior &&
               a.ndata == b.ndata && a.ntail == b.ntail && a.alive == b.alive;
    };
    for (const Case &c : cases) {
        if (c.id <= 0) { fail(c.name, "not created: " + last_error); continue; }
        PcSourceForm f, g, h;
        if (pc_rtc_source_form(c.id, &f) || !same(f, c.want)) fail(c.name, "the form of the live handle");
        const auto hold = pc_rtc_source_hold(c.id, &g);
        if (!hold || !same(g, c.want) || (long long)hold->size() != f.ndata + f.ntail) { fail(c.name, "the hold of the live handle"); continue; }
        pchip_source_destroy(c.id);
        pchip_source_destroy(c.id);
        PcSourceForm dead = c.want;
        dead.alive = 0;
        if (pc_rtc_source_form(c.id, &h) || !same(h, dead)) fail(c.name, "the form after the destroy");
        if (pc_rtc_source_hold(c.id, nullptr)) fail(c.name, "a hold handed out after the destroy");
        // the hold taken before: the doubles that went in, read after the registry let go of them
        bool ok = hold.use_count() == 1;
        for (long i = 0; i < nd; ++i) ok = ok && (*hold)[i] == data[i];
        for (long long i = 0; i < f.ntail; ++i) ok = ok && (*hold)[nd + i] == P[i];
        if (!ok) fail(c.name, "the block behind a hold taken before the destroy");
    }
    PcSourceForm none;
    if (!pc_rtc_source_form(987654, &none) || none.nterms || none.alive) fail("none", "an id that never existed");
    std::printf("%zu handles, %d disagreements\n", sizeof cases / sizeof cases[0], bad);
    return bad ? 1 : 0;
}
