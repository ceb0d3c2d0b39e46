// pc_ini.hip -- ini-file front end: replaces read_params / get_params (src/polychord/ini.f90:44-95,
// 354-458), create_priors + hypercube_to_physical for the prior types used by the shipped examples
// (src/polychord/priors.f90:40-55 uniform, :98-119 log_uniform, :160-183 gaussian, :245-290
// sorted_uniform) and run_polychord_ini (interfaces.F90:232-283, 496-519).
#include "../../include/polychord_hip.h"
#include "pc_prior_table.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <fstream>
#include <sstream>
#include <algorithm>

namespace {

[[noreturn]] void halt_program(const std::string &msg) { std::fprintf(stderr, "%s\n", msg.c_str()); std::exit(1); }

std::string trim(const std::string &s)
{
    const size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

struct Param { std::string name, latex; int speed = 1; std::string prior; int block = 1; std::vector<double> pp; bool sub_cluster = false; };

struct Ini {
    std::vector<std::pair<std::string, std::string>> kv;
    std::vector<Param> params; std::vector<std::pair<std::string, std::string>> derived;
    bool has(const std::string &k) const { for (auto &p : kv) if (p.first == k) return true; return false; }
    std::string str(const std::string &k, const std::string &d) const { for (auto &p : kv) if (p.first == k) return p.second; return d; }
    int integer(const std::string &k, int d) const { return has(k) ? std::atoi(str(k, "").c_str()) : d; }
    int integer_required(const std::string &k) const { if (!has(k)) halt_program("ini error: missing key '" + k + "'"); return integer(k, 0); }
    double dbl(const std::string &k, double d) const { return has(k) ? std::atof(str(k, "").c_str()) : d; }
    bool logical(const std::string &k, bool d) const
    {
        if (!has(k)) return d;
        const std::string v = str(k, "");
        return !v.empty() && (v[0] == 'T' || v[0] == 't' || v == ".true.");
    }
    std::vector<double> dbls(const std::string &k) const
    {
        std::vector<double> out; std::stringstream ss(str(k, "")); double v;
        while (ss >> v) out.push_back(v);
        return out;
    }
};

std::vector<std::string> split_bar(const std::string &s)
{
    std::vector<std::string> out; std::stringstream ss(s); std::string item;
    while (std::getline(ss, item, '|')) out.push_back(trim(item));
    return out;
}

Ini read_ini(const std::string &file)
{
    std::ifstream f(file);
    if (!f) halt_program("ini error: cannot open " + file);
    Ini ini; std::string line;
    while (std::getline(f, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        line = trim(line);
        if (line.empty() || line[0] == '[') continue;
        if ((line[0] == 'P' || line[0] == 'D') && line.find(':') != std::string::npos && trim(line.substr(1, line.find(':') - 1)).empty()) {
            const auto parts = split_bar(line.substr(line.find(':') + 1));
            if (line[0] == 'P') {           // P : name | latex | speed | prior type | prior block | prior params
                if (parts.size() < 6) halt_program("ini error: malformed parameter line: " + line);
                Param p; p.name = parts[0]; p.latex = parts[1]; p.speed = std::atoi(parts[2].c_str()); p.prior = parts[3];
                p.block = std::atoi(parts[4].c_str());
                // sub-clustering marker (ini.f90:389-393): the name cut at its FIRST `*`, the parameter flagged
                const size_t star = p.name.find('*');
                if (star != std::string::npos) { p.name = trim(p.name.substr(0, star)); p.sub_cluster = true; }
                std::stringstream ss(parts[5]); double v; while (ss >> v) p.pp.push_back(v);
                ini.params.push_back(p);
            } else {
                if (parts.size() < 2) halt_program("ini error: malformed derived line: " + line);
                ini.derived.push_back({parts[0], parts[1]});
            }
            continue;
        }
        const size_t eq = line.find('=');
        if (eq == std::string::npos) continue;
        ini.kv.push_back({trim(line.substr(0, eq)), trim(line.substr(eq + 1))});
    }
    return ini;
}

// minimum number of prior parameters of a base type, or -1 if the type is not supported
int base_prior_nparams(const std::string &t)
{
    if (t == "uniform" || t == "log_uniform" || t == "gaussian" || t == "half_gaussian") return 2;
    if (t == "exponential") return 1;
    if (t == "power_uniform") return 3;
    return -1;
}
std::string base_of(const std::string &prior)
{
    if (prior == "nn_adaptive_layer_gaussian") return "gaussian";
    if (prior.rfind("adaptive_sorted_", 0) == 0) return prior.substr(16);
    return prior.rfind("sorted_", 0) == 0 ? prior.substr(7) : prior;
}

// type number of a prior name (priors.f90:5-20), 0 if unknown
int prior_type_of(const std::string &t)
{
    for (int k = 1; k <= 15; ++k) if (t == pc_prior_type_name(k)) return k;
    return 0;
}

// the prior block of the parameter lines as a table (pchip_prior_entry), checked; halts with the reference's words for an unknown type
std::vector<pchip_prior_entry> table_of(const std::vector<Param> &params)
{
    std::vector<pchip_prior_entry> e(params.size());
    for (size_t i = 0; i < params.size(); ++i) {
        const int need = base_prior_nparams(base_of(params[i].prior));
        if (need < 0) halt_program("get_priors error: Unknown prior type for parameter " + params[i].name);
        if ((int)params[i].pp.size() < need) halt_program("ini error: parameter " + params[i].name + " needs " + std::to_string(need) + " prior parameters");
        e[i].type = prior_type_of(params[i].prior); e[i].block = params[i].block; e[i].npar = std::min<int>(3, (int)params[i].pp.size());
        if (pc_prior_is_adaptive(e[i].type)) e[i].npar = (int)params[i].pp.size();      // an adaptive block takes exactly `need`: the true count goes on
        for (int k = 0; k < 3; ++k) e[i].par[k] = k < e[i].npar ? params[i].pp[k] : 0.0;
    }
    return e;
}

// hypercube index of every parameter (priors.f90:708-737): the speeds relabelled 1, 2, 3.. in increasing order, the cube lists the
// parameters grade by grade, file order within a grade; grade_dims = parameters per grade
std::vector<int> hypercube_indices(const std::vector<Param> &params, std::vector<int> *grade_dims = nullptr)
{
    const int nDims = (int)params.size();
    std::vector<int> distinct, hyper((size_t)nDims, 0);
    for (auto &p : params) distinct.push_back(p.speed);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    int h = 0;
    for (size_t g = 0; g < distinct.size(); ++g) {
        int cnt = 0;
        for (int i = 0; i < nDims; ++i) if (params[i].speed == distinct[g]) { hyper[i] = h++; cnt++; }
        if (grade_dims) grade_dims->push_back(cnt);
    }
    return hyper;
}

// settings%sub_clustering_dimensions = pack(hypercube_indices, sub_cluster) (priors.f90:740-741): the marked parameters' cube
// coordinates in PARAMETER order (not sorted), 0-based here
std::vector<int> sub_clustering_dims(const std::vector<Param> &params, const std::vector<int> &hyper)
{
    std::vector<int> out;
    for (size_t i = 0; i < params.size(); ++i) if (params[i].sub_cluster) out.push_back(hyper[i]);
    return out;
}

}  // namespace

std::vector<int> pc_exchange_sub_clustering(const std::vector<int> &dims);      // (pc_abi.hip)

// the sub-clustering list of an ini file (tests; tools): the count, and the first `cap` entries in dims
extern "C" int polychord_hip_ini_sub_clustering(const char *inifile, int *dims, int cap)
{
    const Ini ini = read_ini(inifile ? inifile : "");
    const std::vector<int> sub = sub_clustering_dims(ini.params, hypercube_indices(ini.params));
    for (int k = 0; k < (int)sub.size() && k < cap; ++k) dims[k] = sub[k];
    return (int)sub.size();
}

// AS241 / PPND16 on the host (utils.F90:806-966), the inverse normal CDF every Gaussian prior uses
extern "C" double polychord_hip_inv_normal_cdf(double p) { return pc_inv_normal_cdf_host(p); }

// the prior block of an ini file evaluated at one hypercube point (tests; tools that want theta for a cube sample):
// returns the number of parameters, or -1 when `n` is too small
extern "C" int polychord_hip_ini_prior(const char *inifile, const double *cube, double *theta, int n)
{
    const Ini ini = read_ini(inifile ? inifile : "");
    const int nDims = (int)ini.params.size();
    if (nDims > n) return -1;
    // hypercube order = parameters by speed (priors.f90:708-737), as in polychord_c_interface_ini; the arithmetic is the table's
    // (pc_prior_table.h, the one host implementation).  This helper never checked the prior parameters' values: it still does not
    const std::vector<int> hyper = hypercube_indices(ini.params);
    const std::vector<pchip_prior_entry> e = table_of(ini.params);
    PcPriorTable T;
    T.D = nDims; T.e = e; T.hyper = hyper;
    int stray, head;
    (void)pc_prior_table_blocks(T.e, T.pos, T.len, T.cnt, T.lay, stray, head);
    pc_prior_table_eval(T, cube, theta);
    return nDims;
}

extern "C" void polychord_c_interface_ini(polychord_loglike_fn loglikelihood, void (*setup_loglikelihood)(void), char *inifile, int *comm)
{
    const Ini ini = read_ini(inifile ? inifile : "");
    const int nDims = (int)ini.params.size(), nDerived = (int)ini.derived.size();
    if (nDims == 0) halt_program("ini error: no 'P :' parameter lines");
    if (setup_loglikelihood) setup_loglikelihood();            // interfaces.F90:273
    // uniform-only priors run on the device (when the likelihood is a built-in); anything else is a host prior
    // grades from the speed column (priors.f90:708-737): speeds relabelled 1,2,3.. in increasing order, the hypercube
    // lists the parameters grade by grade (file order within a grade), grade_dims = parameters per grade
    std::vector<int> grade_dims;
    const std::vector<int> hyper = hypercube_indices(ini.params, &grade_dims);
    // the P : lines as a prior table: with a built-in likelihood the run stays on the device whatever the prior types and speeds
    // (polychord_c_interface recognises polychord_hip_table_prior; option "device_prior" = 0: the host function, as before); an
    // all-uniform block in file order is the uniform box
    const std::vector<pchip_prior_entry> entries = table_of(ini.params);
    if (polychord_hip_set_table_prior(nDims, entries.data(), hyper.data()) != 0)
        halt_program(std::string("ini error: ") + (polychord_hip_last_error() ? polychord_hip_last_error() : "bad prior block"));
    bool all_uniform = true;
    std::vector<double> lo(nDims), hi(nDims);
    for (int i = 0; i < nDims; ++i) {
        all_uniform = all_uniform && ini.params[i].prior == "uniform" && hyper[i] == i;
        lo[i] = ini.params[i].pp[0]; hi[i] = ini.params[i].pp.size() > 1 ? ini.params[i].pp[1] : 0.0;
    }
    polychord_prior_fn prior = polychord_hip_table_prior;
    if (all_uniform) { polychord_hip_set_uniform_prior(nDims, lo.data(), hi.data()); prior = polychord_hip_uniform_prior; }
    std::vector<double> grade_frac = ini.dbls("grade_frac");
    if (grade_frac.empty()) grade_frac = {1.0};
    if (grade_frac.size() != grade_dims.size()) {
        if (grade_dims.size() == 1) grade_frac.resize(1);
        else halt_program("ini error: grade_frac needs one entry per parameter speed");
    }
    std::vector<double> loglikes = ini.dbls("loglikes"), nl = ini.dbls("nlives");
    std::vector<int> nlives(nl.begin(), nl.end());
    const int n_nlives = (int)std::min(loglikes.size(), nlives.size());
    std::string base = ini.str("base_dir", "chains"), root = ini.str("file_root", "test");
    // write the .paramnames file (read_write.F90:964+) when asked
    if (ini.logical("write_paramnames", false)) {
        FILE *f = std::fopen((base + "/" + root + ".paramnames").c_str(), "w");
        if (f) {
            for (auto &p : ini.params) std::fprintf(f, "%s      %s\n", p.name.c_str(), p.latex.c_str());
            for (auto &d : ini.derived) std::fprintf(f, "%s*     %s\n", d.first.c_str(), d.second.c_str());
            std::fclose(f);
        }
        f = std::fopen((base + "/" + root + ".properties.ini").c_str(), "w");      // read_write.F90:996-1014
        if (f) { std::fprintf(f, "sampler=nested\nlabel=%s\n", root.c_str()); std::fclose(f); }
    }
    // the markers of this file for this call; the caller's own setting (polychord_hip_set_sub_clustering) back afterwards, whatever happens
    struct SubGuard { std::vector<int> old; ~SubGuard() { pc_exchange_sub_clustering(old); } } sub_guard{pc_exchange_sub_clustering(sub_clustering_dims(ini.params, hyper))};
    polychord_c_interface(loglikelihood, prior, nullptr, ini.integer_required("nlive"), ini.integer_required("num_repeats"),
                          ini.integer("nprior", -1), ini.integer("nfail", -1), ini.logical("do_clustering", false), ini.integer("feedback", 1),
                          ini.dbl("precision_criterion", 1e-3), ini.dbl("logzero", -1e30), ini.integer("max_ndead", -1),
                          ini.dbl("boost_posterior", 0.0), ini.logical("posteriors", false), ini.logical("equals", false),
                          ini.logical("cluster_posteriors", false), ini.logical("write_resume", false), false /* written above with the ini names */,
                          ini.logical("read_resume", false), ini.logical("write_stats", true), ini.logical("write_live", false),
                          ini.logical("write_dead", true), ini.logical("write_prior", false), ini.logical("maximise", false),
                          ini.dbl("compression_factor", std::exp(-1.0)), ini.logical("synchronous", true), nDims, nDerived,
                          (char *)base.c_str(), (char *)root.c_str(), (int)grade_dims.size(), grade_frac.data(), grade_dims.data(), n_nlives,
                          loglikes.empty() ? nullptr : loglikes.data(), nlives.empty() ? nullptr : nlives.data(), ini.integer("seed", -1), comm);
}
