// ref_subclust_driver.cpp -- drives the REFERENCE's ini entry point (polychord_c_interface_ini) with the oracle's likelihoods,
// `random_number` fed from the sequential Philox stream (oracle/ref_rng_shim.c): the only door of the reference through which
// sub-dimension clustering (`*` markers in the ini file) can be asked for.  Built and run by tools/dev/gen_ref_subclust.py on a
// CPU machine, from the objects `make -C oracle ref` leaves in oracle/_ref/obj/; never by a test, smoke() or bench.py.
//
// usage: ref_subclust_driver <like: twin_gaussian | rastrigin | gaussian> <ini file> <seed>
// the run's numbers are then in <base_dir>/<file_root>.stats of the ini file
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <sys/resource.h>
extern "C" {
#include "pc_oracle.h"
}

extern "C" void polychord_c_interface_ini(double (*)(double *, int, double *, int), void (*)(), char *, int &);
extern "C" void pc_shim_reset(unsigned);

static pc_like g_like;
static double loglike(double *theta, int nDims, double *phi, int nDerived) { return pc_like_eval(&g_like, theta, nDims, phi, nDerived); }
static void setup() {}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s like inifile seed\n", argv[0]); return 2; }
    struct rlimit rl; getrlimit(RLIMIT_STACK, &rl); rl.rlim_cur = rl.rlim_max; setrlimit(RLIMIT_STACK, &rl);
    std::memset(&g_like, 0, sizeof g_like);
    const std::string like = argv[1];
    if (like == "twin_gaussian") { g_like.kind = PC_LIKE_TWIN_GAUSSIAN; g_like.sigma = 0.1; }
    else if (like == "rastrigin") g_like.kind = PC_LIKE_RASTRIGIN;
    else if (like == "gaussian") { g_like.kind = PC_LIKE_GAUSSIAN; g_like.mu = 0.5; g_like.sigma = 0.1; }
    else { std::fprintf(stderr, "unknown likelihood %s\n", argv[1]); return 2; }
    // the Fortran side reads the file name as character(len=1), dimension(STR_LENGTH = 300) (interfaces.F90:510): a padded buffer
    std::vector<char> ini(300, ' ');
    const size_t n = std::strlen(argv[2]);
    if (n >= ini.size()) { std::fprintf(stderr, "ini path too long\n"); return 2; }
    std::memcpy(ini.data(), argv[2], n);
    ini[n] = '\0';
    pc_shim_reset((unsigned)std::atoi(argv[3]));
    int comm = 0;
    polychord_c_interface_ini(loglike, setup, ini.data(), comm);
    return 0;
}
