// pc_source.hip -- a device-source handle evaluated on its own, outside a run: pchip_source_eval, pchip_source_prior_eval, and the batch
// evaluator behind the PolyChord-interface doors (a source likelihood under a HOST prior).  None of them touches an Engine: each finds the
// handle, puts its data block on the device (SourceBlock) and launches k_source_eval / k_prior_transform of the handle's run-time module.
#include "pc_state.h"
#include "pc_launch.h"
#include "../../include/polychord_hip.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

namespace {

// A live handle's data block resident on the current device, as a run uploads it: the user's form.ndata doubles and the form.ntail of the
// handle's own behind them (a quadratic form's matrix) in one piece.  find: the hold (false: no such handle, or destroyed); upload: allocate
// and copy, waited for, and the hold goes; the destructor frees.  d stays NULL for a handle without data.
struct SourceBlock {
    PcSourceForm form{};
    std::shared_ptr<const std::vector<double>> hold;
    double *d = nullptr;
    bool find(int handle) { hold = pc_rtc_source_hold(handle, &form); return hold != nullptr; }
    bool upload(hipStream_t st)
    {
        const size_t nb = sizeof(double) * hold->size();
        bool ok = nb == 0 || hipMalloc(&d, nb) == hipSuccess;
        if (ok && nb) ok = st ? hipMemcpyAsync(d, hold->data(), nb, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess
                              : hipMemcpy(d, hold->data(), nb, hipMemcpyHostToDevice) == hipSuccess;
        hold.reset();
        return ok;
    }
    SourceBlock() = default; SourceBlock(const SourceBlock &) = delete;
    ~SourceBlock() { if (d) (void)hipFree(d); }
    // the state of a kernel launched outside a run: the handle, its block, nothing else
    PcState state(int handle, int nDims, int nDerived) const
    {
        PcState S; std::memset(&S, 0, sizeof(S));
        S.D = nDims; S.nDer = nDerived; S.like.kind = PC_LIKE_SOURCE; S.src_id = handle; S.src_data = d; S.src_ndata = form.ndata;
        return S;
    }
};

std::string no_handle(const char *who, int handle) { return std::string(who) + "device source handle " + std::to_string(handle) + " does not exist"; }
bool no_device()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return false;
    (void)hipGetLastError();
    std::fprintf(stderr, "polychord_hip: no HIP device available -- this engine has no CPU path\n");
    return true;
}

}  // namespace

extern "C" {

// the prior of a source handle alone at n hypercube points: the handle's run-time module, k_prior_transform, one wavefront a point
// (the whole block goes up, a quadratic form's matrix included: the prior never reads the tail, and one way of uploading is enough)
int pchip_source_prior_eval(int handle, const double *cubes, long n, int nDims, double *thetas)
{
    SourceBlock B;
    if (!B.find(handle)) { pc_abi_set_last_error(no_handle("pchip_source_prior_eval: ", handle).c_str()); return 1; }
    if (!B.form.has_prior) { pc_abi_set_last_error(("pchip_source_prior_eval: device source handle " + std::to_string(handle) + " defines no pchip_prior_param (pchip_source_create_prior makes one that does)").c_str()); return 1; }
    if (!cubes || !thetas || n < 1 || n > 0x7fffffffL || nDims < 1) { pc_abi_set_last_error("pchip_source_prior_eval: n >= 1 points, nDims >= 1, arrays for cube and theta"); return 1; }
    if (nDims > 256) return 3;
    if (no_device()) return 2;
    double *d_c = nullptr, *d_t = nullptr;
    const size_t nb = sizeof(double) * (size_t)n * nDims;
    int rc = 2;
    pc_abi_set_last_error(nullptr);
    if (B.upload(nullptr) && hipMalloc(&d_c, nb) == hipSuccess && hipMalloc(&d_t, nb) == hipSuccess && hipMemcpy(d_c, cubes, nb, hipMemcpyHostToDevice) == hipSuccess) {
        PcState S = B.state(handle, nDims, 0);
        S.prior.kind = PCHIP_PRIOR_SOURCE;
        if (pc_launch_source_prior_eval(&S, (int)n, d_c, d_t, nullptr)) { rc = 1; pc_abi_set_last_error(pc_rtc_error() ? pc_rtc_error() : "pchip_source_prior_eval: the launch failed"); }
        else if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(thetas, d_t, nb, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
    }
    if (rc == 2) (void)hipGetLastError();
    (void)hipFree(d_c); (void)hipFree(d_t);
    return rc;
}

// a source likelihood alone at n points (any form of source): the handle's run-time module, k_source_eval, one wavefront a point
int pchip_source_eval(int handle, const double *thetas, long n, int nDims, int nDerived, double *logL, double *phi)
{
    SourceBlock B;
    if (!B.find(handle)) { pc_abi_set_last_error(no_handle("pchip_source_eval: ", handle).c_str()); return 1; }
    if (!thetas || !logL || n < 1 || n > 0x7fffffffL || nDims < 1 || nDerived < 0 || (nDerived > 0 && !phi)) {
        pc_abi_set_last_error("pchip_source_eval: n >= 1 points, nDims >= 1, arrays for theta, logL and (nDerived > 0) phi"); return 1;
    }
    if (nDerived > PC_SRC_MAX_DERIVED) { pc_abi_set_last_error(("pchip_source_eval: a device source likelihood writes at most " + std::to_string(PC_SRC_MAX_DERIVED) + " derived parameters").c_str()); return 1; }
    if (nDims > 256) return 3;
    if (no_device()) return 2;
    double *d_t = nullptr, *d_l = nullptr, *d_p = nullptr, *d_R = nullptr, *d_part = nullptr;
    const size_t nt = sizeof(double) * (size_t)n * nDims, np = sizeof(double) * (size_t)n * (nDerived > 0 ? nDerived : 1);
    int rc = 2;
    pc_abi_set_last_error(nullptr);
    // (the batched quadratic form: the evaluator of its runs, slab by slab -- scratch for the residuals and the partial sums of a slab)
    const int nres = B.form.nbatch;
    const long slab = std::min<long>(n, PC_QUAD_BATCH_SLAB), srows = pc_quad_mm_rows(slab);
    const bool scratch = nres <= 0 || (hipMalloc(&d_R, sizeof(double) * (size_t)srows * pc_quad_mm_ldr(nres)) == hipSuccess &&
                                       hipMalloc(&d_part, sizeof(double) * (size_t)srows * pc_quad_mm_ncb(nres)) == hipSuccess);
    if (scratch && B.upload(nullptr) && hipMalloc(&d_t, nt) == hipSuccess && hipMalloc(&d_l, sizeof(double) * (size_t)n) == hipSuccess && hipMalloc(&d_p, np) == hipSuccess &&
        hipMemcpy(d_t, thetas, nt, hipMemcpyHostToDevice) == hipSuccess) {
        const PcState S = B.state(handle, nDims, nDerived);
        int failed = 0;
        if (nres > 0) {
            for (long at = 0; at < n && !failed; at += slab)
                failed = pc_launch_quad_batch(&S, nres, (int)std::min(slab, n - at), d_t + (size_t)at * nDims, d_l + at, d_p + (size_t)at * nDerived, d_R, d_part, nullptr);
        } else failed = pc_launch_source_eval(&S, (int)n, d_t, d_l, d_p, nullptr);
        if (failed) { rc = 1; pc_abi_set_last_error(pc_rtc_error() ? pc_rtc_error() : "pchip_source_eval: the launch failed"); }
        else if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(logL, d_l, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess &&
                 (nDerived == 0 || hipMemcpy(phi, d_p, np, hipMemcpyDeviceToHost) == hipSuccess)) rc = 0;
    }
    if (rc == 2) (void)hipGetLastError();
    (void)hipFree(d_t); (void)hipFree(d_l); (void)hipFree(d_p); (void)hipFree(d_R); (void)hipFree(d_part);
    return rc;
}

// The batched quadratic form at the doors that start work on a likelihood / prior pair: what it cannot do, said before any device call.
// who: the entry point (pchip_run, pchip_run_in_step: a device prior is all they need; any other name: the handle is not taken at all)
const char *pc_quad_batch_refusal(const char *who, const pchip_like *like, const pchip_prior *prior, int *nres)
{
    thread_local std::string msg;
    if (nres) *nres = 0;
    PcSourceForm f;
    if (!like || like->kind != PCHIP_LIKE_SOURCE || pc_rtc_source_form(like->source, &f) != 0 || f.nbatch <= 0) return nullptr;
    if (nres) *nres = f.nbatch;
    const std::string me = std::string(who) + ": device source handle " + std::to_string(like->source) + " is a batched quadratic form (pchip_source_create_quad_batch)";
    const bool runs = std::strcmp(who, "pchip_run") == 0 || std::strcmp(who, "pchip_run_in_step") == 0;
    if (!runs) { msg = me + " -- not covered: it is evaluated in batches on the matrix cores, by pchip_run, pchip_run_in_step and pchip_source_eval alone"; return msg.c_str(); }
    if (prior && prior->kind == PCHIP_PRIOR_SOURCE) { msg = me + " and has no prior of its own -- prior.kind = 3 (source prior) is refused: the uniform box (1) or a table (2)"; return msg.c_str(); }
    if (prior && prior->kind != 1 && prior->kind != PCHIP_PRIOR_TABLE) { msg = me + " -- its blocks stay on the device: a host prior (prior.kind = " + std::to_string(prior->kind) + ") is refused, the uniform box (1) or a table (2)"; return msg.c_str(); }
    return nullptr;
}

// ---- a source likelihood under a HOST prior, for the PolyChord-interface doors (pc_abi.hip) ------------------------------------------
// pchip_run refuses that pair (a source has no host function of its own to run callback mode through); the doors run callback mode with
// polychord_hip_source_loglike and register this evaluator as the batch callback for the length of their call: the parked proposals of a
// round get the host prior one by one, on the calling thread, and ONE launch of k_source_eval for all of them -- the bits of
// pchip_source_eval at each point (one wavefront a point, whatever n).  Opened once per run: the handle's data block (a quadratic form's
// matrix behind it) stays on the device, the theta / logL / phi buffers grow on demand, the copies and the launch go through a stream of
// its own and only that stream is waited for.
struct PcSourceBatch {
    int handle = 0, D = 0, nDer = 0;
    polychord_prior_fn prior = nullptr;
    hipStream_t st = nullptr;
    SourceBlock src;
    double *d_buf = nullptr, *h_buf = nullptr;      // [cap] rows of theta (D) | logL (1) | phi (max(1, nDer)): device, and pinned host
    long cap = 0;
    bool failed = false;
    size_t row() const { return (size_t)D + 1 + (size_t)(nDer > 0 ? nDer : 1); }
    bool grow(long n)
    {
        if (n <= cap) return true;
        const long want = std::max(n, 2 * cap);
        (void)hipFree(d_buf); (void)hipHostFree(h_buf); d_buf = h_buf = nullptr; cap = 0;
        if (hipMalloc(&d_buf, sizeof(double) * row() * (size_t)want) != hipSuccess || hipHostMalloc(&h_buf, sizeof(double) * row() * (size_t)want) != hipSuccess) return false;
        cap = want;
        return true;
    }
};

void *pc_source_batch_open(int handle, int device, int nDims, int nDerived, polychord_prior_fn prior)
{
    PcSourceBatch *b = new PcSourceBatch;
    auto refuse = [b](const std::string &msg) { pc_abi_set_last_error(msg.c_str()); pc_source_batch_close(b); return (void *)nullptr; };
    if (!b->src.find(handle)) return refuse(no_handle("", handle));
    if (b->src.form.nbatch > 0) return refuse("device source handle " + std::to_string(handle) + " is a batched quadratic form (pchip_source_create_quad_batch): a host prior is refused, the uniform box or a prior table");
    if (!prior || nDims < 1 || nDims > 256 || nDerived < 0 || nDerived > PC_SRC_MAX_DERIVED) return refuse("a source likelihood under a host prior: a prior function, 1 <= nDims <= 256, 0 <= nDerived <= 32");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return refuse("no HIP device available -- this engine has no CPU path"); }
    b->handle = handle; b->D = nDims; b->nDer = nDerived; b->prior = prior;
    if (!(hipSetDevice(device >= 0 ? device % ndev : 0) == hipSuccess && hipStreamCreate(&b->st) == hipSuccess && b->src.upload(b->st))) {
        (void)hipGetLastError(); return refuse("a source likelihood under a host prior: the stream or the data block could not be set up on the device");
    }
    return b;
}

void pc_source_batch_close(void *user)
{
    PcSourceBatch *b = (PcSourceBatch *)user;
    if (!b) return;
    if (b->st) { (void)hipStreamSynchronize(b->st); (void)hipStreamDestroy(b->st); }
    (void)hipFree(b->d_buf); (void)hipHostFree(b->h_buf);
    delete b;
}

// (a polychord_batch_fn: `user` is the evaluator)
void pc_source_batch_eval(void *user, int n, int nDims, int nDerived, const double *cube, double *theta, double *phi, double *logL)
{
    PcSourceBatch *b = (PcSourceBatch *)user;
    const int D = b->D, nDer = b->nDer, pd = nDer > 0 ? nDer : 1;
    if (n < 1) return;
    for (int i = 0; i < n; ++i) b->prior(const_cast<double *>(cube) + (size_t)i * D, theta + (size_t)i * D, D);
    bool ok = !b->failed && nDims == D && nDerived == nDer && b->grow(n);
    if (ok) {
        double *h_t = b->h_buf, *h_l = h_t + (size_t)n * D, *h_p = h_l + n;
        double *d_t = b->d_buf, *d_l = d_t + (size_t)n * D, *d_p = d_l + n;
        std::memcpy(h_t, theta, sizeof(double) * (size_t)n * D);
        const PcState S = b->src.state(b->handle, D, nDer);
        ok = hipMemcpyAsync(d_t, h_t, sizeof(double) * (size_t)n * D, hipMemcpyHostToDevice, b->st) == hipSuccess;
        if (ok && pc_launch_source_eval(&S, n, d_t, d_l, d_p, b->st)) { ok = false; pc_abi_set_last_error(pc_rtc_error() ? pc_rtc_error() : "a source likelihood under a host prior: k_source_eval could not be launched"); }
        else if (ok) {
            ok = hipMemcpyAsync(h_l, d_l, sizeof(double) * ((size_t)n + (size_t)n * pd), hipMemcpyDeviceToHost, b->st) == hipSuccess && hipStreamSynchronize(b->st) == hipSuccess;
            if (!ok) pc_abi_set_last_error((std::string("a source likelihood under a host prior: HIP error ") + hipGetErrorString(hipGetLastError())).c_str());
        }
        if (ok) {
            std::memcpy(logL, h_l, sizeof(double) * (size_t)n);
            if (nDer > 0) std::memcpy(phi, h_p, sizeof(double) * (size_t)n * nDer);
        }
    } else if (!b->failed) pc_abi_set_last_error("a source likelihood under a host prior: the buffers of a round could not be allocated");
    if (!ok) {      // no value to give: every point invalid, and the run stops at this host boundary (the message stays in polychord_hip_last_error)
        if (!b->failed && polychord_hip_last_error()) std::fprintf(stderr, "polychord_hip: %s\n", polychord_hip_last_error());
        b->failed = true;
        for (int i = 0; i < n; ++i) logL[i] = -1.7976931348623157e308;
        for (size_t i = 0; i < (size_t)n * pd; ++i) phi[i] = 0.0;
        polychord_hip_request_stop();
    }
}

}  // extern "C"
