// device_batch_gauss.hip -- a likelihood that lives on the GPU, behind polychord_hip_set_device_batch_callback, and its host twin.
// tests/test_device_batch.py and tools/dev/bench_device_batch.py build it into a shared object of their own:
//
//     hipcc --offload-arch=gfx950 -O2 -fPIC -shared -ffp-contract=off device_batch_gauss.hip -o libdbgauss.so
//
// logL = -0.5 * sum_d ((theta_d - mu) / sigma)^2 + c, summed in the order of d, phi_0 = the sum, theta = cube (the callback owns the
// prior: the unit box) unless flags bit 0 says the engine has filled theta.  One formula, written once, compiled for both sides with
// contraction off: + - * / are correctly rounded on either, so the device callback's run and the host twin's are one run, bit for bit.
// The device callback launches ONE kernel on the engine's stream and returns without waiting: that run is the right one only if the
// engine orders its pack in front of the kernel and its next tick behind it.
//
// `inner` > 0 repeats the sum that many times (the bench's dear end); the value is that of one pass.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

struct GaussCtx { double mu, sigma, c; int inner; int calls; };

__host__ __device__ static inline double gauss_row(const double *cube, double *theta, int D, int own_prior, double mu, double sigma, double c, int inner,
                                                   double *sum_out)
{
    double s = 0.0;
    for (int pass = 0; pass <= inner; ++pass) {
        s = 0.0;
        for (int d = 0; d < D; ++d) {
            double t;
            if (own_prior) { t = cube[d]; theta[d] = t; } else t = theta[d];
            const double z = (t - mu) / sigma;
            s = s + z * z;
        }
#if defined(__HIP_DEVICE_COMPILE__)
        __asm__ volatile("" : "+v"(s));      // (the passes are not folded into one)
#endif
    }
    *sum_out = s;
    return -0.5 * s + c;
}

__global__ void k_gauss_rows(int n, int D, int nDer, const double *cube, double *theta, double *phi, double *logL, int flags, double mu, double sigma,
                             double c, int inner)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s;
    logL[i] = gauss_row(cube + (size_t)i * D, theta + (size_t)i * D, D, !(flags & 1), mu, sigma, c, inner, &s);
    if (nDer > 0) phi[(size_t)i * nDer] = s;
    for (int e = 1; e < nDer; ++e) phi[(size_t)i * nDer + e] = 0.0;
}

extern "C" {

// polychord_device_batch_fn: one launch on `stream`, no wait
int gauss_device_batch(void *user, int n, int nDims, int nDerived, const double *d_cube, double *d_theta, double *d_phi, double *d_logL, int flags,
                       void *stream)
{
    GaussCtx *g = (GaussCtx *)user;
    g->calls++;
    hipLaunchKernelGGL(k_gauss_rows, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, n, nDims, nDerived, d_cube, d_theta, d_phi, d_logL, flags,
                       g->mu, g->sigma, g->c, g->inner);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// polychord_batch_fn: the host twin, the same rows on the calling thread
void gauss_host_batch(void *user, int n, int nDims, int nDerived, const double *cube, double *theta, double *phi, double *logL)
{
    GaussCtx *g = (GaussCtx *)user;
    g->calls++;
    for (int i = 0; i < n; ++i) {
        double s;
        logL[i] = gauss_row(cube + (size_t)i * nDims, theta + (size_t)i * nDims, nDims, 1, g->mu, g->sigma, g->c, 0, &s);
        if (nDerived > 0) phi[(size_t)i * nDerived] = s;
        for (int e = 1; e < nDerived; ++e) phi[(size_t)i * nDerived + e] = 0.0;
    }
}

// what a user writes around a GPU likelihood TODAY, behind the host batch callback: cubes up, one launch, answers down (the bench's path a).
// user: GaussCtx followed by nothing -- the staging blocks are this file's, grown on demand.
static double *g_dc = nullptr, *g_dt = nullptr, *g_dp = nullptr, *g_dl = nullptr; static size_t g_cap = 0;
void gauss_host_batch_via_device(void *user, int n, int nDims, int nDerived, const double *cube, double *theta, double *phi, double *logL)
{
    GaussCtx *g = (GaussCtx *)user;
    g->calls++;
    const int pd = nDerived > 0 ? nDerived : 1;
    if ((size_t)n > g_cap) {
        (void)hipFree(g_dc); (void)hipFree(g_dt); (void)hipFree(g_dp); (void)hipFree(g_dl);
        g_cap = (size_t)n * 2;
        (void)hipMalloc(&g_dc, sizeof(double) * g_cap * nDims); (void)hipMalloc(&g_dt, sizeof(double) * g_cap * nDims);
        (void)hipMalloc(&g_dp, sizeof(double) * g_cap * pd); (void)hipMalloc(&g_dl, sizeof(double) * g_cap);
    }
    (void)hipMemcpy(g_dc, cube, sizeof(double) * (size_t)n * nDims, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_gauss_rows, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t) nullptr, n, nDims, nDerived, (const double *)g_dc, g_dt, g_dp, g_dl, 0,
                       g->mu, g->sigma, g->c, g->inner);
    (void)hipMemcpy(theta, g_dt, sizeof(double) * (size_t)n * nDims, hipMemcpyDeviceToHost);
    (void)hipMemcpy(phi, g_dp, sizeof(double) * (size_t)n * pd, hipMemcpyDeviceToHost);
    (void)hipMemcpy(logL, g_dl, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
}
void gauss_release(void) { (void)hipFree(g_dc); (void)hipFree(g_dt); (void)hipFree(g_dp); (void)hipFree(g_dl); g_dc = g_dt = g_dp = g_dl = nullptr; g_cap = 0; }

// the scalar callbacks a run still needs (single evaluations, the maximiser): the unit box and the same formula
static GaussCtx g_scalar = {0.5, 0.1, 0.0, 0, 0};
void gauss_set_scalar(double mu, double sigma, double c) { g_scalar.mu = mu; g_scalar.sigma = sigma; g_scalar.c = c; }
void gauss_prior(double *cube, double *theta, int nDims) { for (int d = 0; d < nDims; ++d) theta[d] = cube[d]; }
double gauss_loglike(double *theta, int nDims, double *phi, int nDerived)
{
    double s;
    const double l = gauss_row(theta, theta, nDims, 0, g_scalar.mu, g_scalar.sigma, g_scalar.c, 0, &s);
    if (nDerived > 0) phi[0] = s;
    for (int e = 1; e < nDerived; ++e) phi[e] = 0.0;
    return l;
}

}
