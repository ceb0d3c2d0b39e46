// polychord_hip_cli -- runs an ini file through polychord_c_interface_ini with one of the built-in
// device likelihoods, or with a likelihood written as device source; counterpart of the reference's
// src/drivers/polychord_CC_ini.cpp:10-18.
//   usage: polychord_hip_cli <file.ini> <gaussian|rastrigin|twin_gaussian|source:FILE> [batch] [option=value ...]
//                            [data:FILE] [nterms:N] [nsums:K] [shared:N]
//   (option=value: polychord_hip_set_option, e.g. device_prior=0 -- the ini file's prior block on the host)
//   source:FILE -- FILE holds the HIP source text of the likelihood (pchip_source_create; polychord_hip.h).  data:FILE -- its data
//   block, raw little-endian float64.  nterms:N -- the terms form of N terms (pchip_source_create_terms); nsums:K with it -- K sums per
//   evaluation (pchip_source_create_sums).  shared:N with nterms: -- N shared values per point (pchip_source_create_shared: the text
//   defines pchip_shared_value and its form's functions with `shared` behind theta).
#include "polychord_hip.h"
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include <sys/stat.h>

static const char *USAGE = "usage: %s <file.ini> <gaussian|rastrigin|twin_gaussian|source:FILE> [batch] [option=value ...] [data:FILE] [nterms:N] [nsums:K] [shared:N]\n";

static bool read_file(const char *path, std::string &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    const bool ok = !std::ferror(f);
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, USAGE, argv[0]); return 2; }
    polychord_loglike_fn like = nullptr;
    const char *source_path = nullptr, *data_path = nullptr;
    long nterms = 0, nshared = 0; int nsums = 0; bool shared = false;
    if (!std::strcmp(argv[2], "gaussian")) like = polychord_hip_gaussian;
    else if (!std::strcmp(argv[2], "rastrigin")) like = polychord_hip_rastrigin;
    else if (!std::strcmp(argv[2], "twin_gaussian")) like = polychord_hip_twin_gaussian;
    else if (!std::strncmp(argv[2], "source:", 7)) { like = polychord_hip_source_loglike; source_path = argv[2] + 7; }
    else { std::fprintf(stderr, "unknown likelihood %s\n", argv[2]); return 2; }
    for (int a = 3; a < argc; ++a) {
        if (!std::strncmp(argv[a], "data:", 5)) { data_path = argv[a] + 5; continue; }
        if (!std::strncmp(argv[a], "nterms:", 7)) { nterms = std::atol(argv[a] + 7); continue; }
        if (!std::strncmp(argv[a], "nsums:", 6)) { nsums = std::atoi(argv[a] + 6); continue; }
        if (!std::strncmp(argv[a], "shared:", 7)) { nshared = std::atol(argv[a] + 7); shared = true; continue; }
        char *eq = std::strchr(argv[a], '=');
        if (eq) { *eq = 0; polychord_hip_set_option(argv[a], std::atof(eq + 1)); }
        else polychord_hip_set_option("batch", std::atof(argv[a]));
    }
    int handle = 0;
    if (source_path) {
        std::string text, raw;
        if (!read_file(source_path, text)) { std::fprintf(stderr, "%s: cannot read the source file %s\n", argv[0], source_path); return 2; }
        if (data_path && !read_file(data_path, raw)) { std::fprintf(stderr, "%s: cannot read the data file %s\n", argv[0], data_path); return 2; }
        if (raw.size() % sizeof(double)) { std::fprintf(stderr, "%s: %s holds %zu bytes, not a whole number of float64\n", argv[0], data_path, raw.size()); return 2; }
        std::vector<double> data(raw.size() / sizeof(double));
        if (!data.empty()) std::memcpy(data.data(), raw.data(), raw.size());
        const double *d = data.empty() ? nullptr : data.data();
        const long nd = (long)data.size();
        if (shared) handle = pchip_source_create_shared(text.c_str(), nullptr, d, nd, nshared, nterms, nsums, 0, nullptr, 0);
        else if (nsums > 0) handle = pchip_source_create_sums(text.c_str(), nullptr, d, nd, nterms, nsums, 0);
        else if (nterms > 0) handle = pchip_source_create_terms(text.c_str(), nullptr, d, nd, nterms);
        else handle = pchip_source_create(text.c_str(), nullptr, d, nd);
        if (handle <= 0 || polychord_hip_set_source(handle) != 0) {
            const char *log = polychord_hip_last_error();
            std::fprintf(stderr, "%s: the source of %s was refused:\n%s\n", argv[0], source_path, log ? log : "(no message)");
            return 2;
        }
    } else if (data_path || nterms || nsums || shared) { std::fprintf(stderr, "%s: data:, nterms:, nsums: and shared: go with source:FILE\n", argv[0]); return 2; }
    mkdir("chains", 0755); mkdir("chains/clusters", 0755);
    int comm = 0;
    polychord_c_interface_ini(like, nullptr, argv[1], &comm);
    if (handle > 0) { polychord_hip_set_source(0); pchip_source_destroy(handle); }
    return 0;
}
