// The driver of example_gaussian.cpp with the likelihood written as device source: the text is compiled at run time for the GPU the
// run is on and evaluated inside the sampling kernel, like the built-in Gaussian -- files, dumper and `maximise` as for any run.
//   g++ -std=c++17 -I include bindings/cpp/example_source.cpp -L polychordlite_amd -lpolychord_hip -Wl,-rpath,$PWD/polychordlite_amd
#include <cmath>
#include <cstdio>
#include "polychord_hip.hpp"

// likelihoods/examples/gaussian.f90: N(0.5, 0.1^2 I), phi_1 = radius
static const char *SOURCE = R"(
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    double r2 = 0.0;
    for (int i = 0; i < nDims; ++i) r2 += (theta[i] - data[0]) * (theta[i] - data[0]);
    if (nDerived > 0) phi[0] = sqrt(r2);
    return -nDims * (log(data[1]) + 0.5 * log(6.283185307179586)) - 0.5 * r2 / (data[1] * data[1]);
}
)";

static int g_dumps = 0;
static void my_dumper(int ndead, int nlive, int npars, double *, double *, double *, double logZ, double logZerr)
{
    ++g_dumps;
    if (nlive == 0) std::printf("final dump: ndead %d npars %d logZ %.4f +/- %.4f\n", ndead, npars, logZ, logZerr);
}

int main(int argc, char **argv)
{
    const double data[2] = { 0.5, 0.1 };      // mu, sigma: the handle's data block
    const int handle = pchip_source_create(SOURCE, nullptr, data, 2);
    if (handle <= 0 || polychord_hip_set_source(handle) != 0) {
        std::fprintf(stderr, "%s\n", polychord_hip_last_error() ? polychord_hip_last_error() : "the source was refused");
        return 2;
    }
    double theta[6] = { 0.5, 0.5, 0.5, 0.5, 0.5, 0.6 }, phi[1];
    std::printf("logL at one point, through the host function: %.6f (radius %.3f)\n", polychord_hip_source_loglike(theta, 6, phi, 1), phi[0]);
    Settings s(6, 1);
    s.nlive = 120; s.num_repeats = 12; s.seed = 3; s.feedback = 0; s.write_stats = true; s.write_prior = false;
    s.base_dir = argc > 1 ? argv[1] : "chains"; s.file_root = "cpp_source";
    run_polychord(polychord_hip_source_loglike, polychord_hip_uniform_prior, my_dumper, s);     // fused on the GPU; maximise on the device
    polychord_hip_set_source(0);
    pchip_source_destroy(handle);
    return g_dumps > 2 ? 0 : 1;
}
