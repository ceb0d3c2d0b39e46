// pc_maximise.hip -- `maximise = T`: polish the best live points into the maximum-likelihood and maximum-posterior points
// and write <root>.maximum.
//
// Restates maximise / do_maximisation / dXdtheta (reference src/polychord/maximiser.F90:32-224), nelder_mead
// (src/polychord/nelder_mead.f90:7-83) and write_max_file (src/polychord/read_write.F90:754-807).  Host code: a simplex of
// nDims + 1 points and a few hundred likelihood calls, made through the same prior / loglikelihood callbacks as the run
// (the built-in device likelihoods are ordinary host functions too, include/polychord_hip.h).  It runs on the live set
// at termination, before the final kill-off, like the reference (nested_sampling.F90:379).
#include "pc_launch.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

namespace {

// determinant by elimination with row swaps on zero pivots (nelder_mead.f90:168-209; column-major n x n, destroyed)
double det_cm(std::vector<double> &M, int n)
{
    int sign = 1;
    auto at = [&](int r, int c) -> double & { return M[(size_t)c * n + r]; };
    for (int k = 0; k < n - 1; ++k) {
        if (at(k, k) == 0.0) {
            bool found = false;
            for (int i = k + 1; i < n; ++i)
                if (at(i, k) != 0.0) {
                    for (int j = 0; j < n; ++j) std::swap(at(i, j), at(k, j));
                    found = true; sign = -sign;
                    break;
                }
            if (!found) return 0.0;
        }
        for (int j = k + 1; j < n; ++j) {
            const double m = at(j, k) / at(k, k);
            for (int i = k + 1; i < n; ++i) at(j, i) -= m * at(k, i);
        }
    }
    double d = sign;
    for (int i = 0; i < n; ++i) d *= at(i, i);
    return d;
}

// simplex x[n+1][n] (one point per row), values f[n+1]; maximises func; returns the best vertex (nelder_mead.f90:7-83)
std::vector<double> nelder_mead(const std::function<double(const double *)> &func, std::vector<double> x, std::vector<double> f, double dl, long *niter)
{
    const int n = (int)f.size() - 1;
    const double alpha = 1.0, gamma = 2.0, rho = 0.5, sigma = 0.5;
    std::vector<int> idx(n + 1);
    std::vector<double> xo(n), xr(n), xe(n), xc(n), E((size_t)n * n);
    double det0 = -1.0;
    auto P = [&](int v) { return x.data() + (size_t)v * n; };
    for (int iter = 0; iter < 200000; ++iter) {
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return f[a] < f[b]; });      // ascending: idx[0] worst, idx[n] best
        for (int c = 0; c < n; ++c) for (int r = 0; r < n; ++r) E[(size_t)c * n + r] = P(idx[c])[r] - P(idx[n])[r];   // edges from the best vertex
        const double det1 = std::fabs(det_cm(E, n));
        if (det0 < 0.0) det0 = det1;
        if (f[idx[n]] - f[idx[0]] < dl || !(det0 > 0.0) || std::pow(det1 / det0, 1.0 / n) < dl) break;
        for (int r = 0; r < n; ++r) { double s = 0.0; for (int k = 1; k <= n; ++k) s += P(idx[k])[r]; xo[r] = s / n; }   // centroid of all but the worst
        const int w = idx[0];
        ++*niter;
        for (int r = 0; r < n; ++r) xr[r] = xo[r] + alpha * (xo[r] - P(w)[r]);
        const double fr = func(xr.data());
        if (fr <= f[idx[n]] && f[idx[1]] < fr) { f[w] = fr; std::copy(xr.begin(), xr.end(), P(w)); }
        else if (fr > f[idx[n]]) {                                       // expansion
            for (int r = 0; r < n; ++r) xe[r] = xo[r] + gamma * (xr[r] - xo[r]);
            const double fe = func(xe.data());
            if (fe > fr) { f[w] = fe; std::copy(xe.begin(), xe.end(), P(w)); } else { f[w] = fr; std::copy(xr.begin(), xr.end(), P(w)); }
        } else {                                                          // contraction, else shrink towards the best
            for (int r = 0; r < n; ++r) xc[r] = xo[r] + rho * (P(w)[r] - xo[r]);
            const double fc = func(xc.data());
            if (fc > f[w]) { f[w] = fc; std::copy(xc.begin(), xc.end(), P(w)); }
            else for (int j = 0; j < n; ++j) {
                const int v = idx[j];
                for (int r = 0; r < n; ++r) P(v)[r] = P(idx[n])[r] + sigma * (P(v)[r] - P(idx[n])[r]);
                f[v] = func(P(v));
            }
        }
    }
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return f[a] < f[b]; });
    return std::vector<double>(P(idx[n]), P(idx[n]) + n);
}

std::string e24(double v)
{   // Fortran E24.15E3:  "  0.626931681801488E-001"
    char buf[64];
    if (v == 0.0 || !std::isfinite(v)) {
        if (!std::isfinite(v)) { std::snprintf(buf, sizeof buf, "%24s", std::isnan(v) ? "NaN" : (v > 0 ? "Infinity" : "-Infinity")); return buf; }
        return std::string("   0.000000000000000E+000");
    }
    char t[64];
    std::snprintf(t, sizeof t, "%.14E", std::fabs(v));     // d.ddddddddddddddE+XX
    const char *e = std::strchr(t, 'E');
    const int ex = std::atoi(e + 1) + 1;
    std::string digits;
    digits += t[0];
    digits.append(t + 2, 14);
    std::snprintf(buf, sizeof buf, "%s0.%sE%c%03d", v < 0 ? "-" : "", digits.c_str(), ex < 0 ? '-' : '+', std::abs(ex));
    char out[64];
    std::snprintf(out, sizeof out, "%24s", buf);
    return out;
}

}  // namespace

// ---- the choice of simplex, the values, the writer: one copy each, for the host maximiser here and the device maximiser (pc_engine.hip) ----

// do_maximisation's choice (maximiser.F90:92-161).  live: [nlive][nTotal] rows [cube | theta | phi | birth | logL]; cluster: [nlive] labels;
// vals: the candidate value of every row (NULL: its logL)
extern "C" int pc_max_choose_simplex(int D, int nT, double logzero, const double *live, const int *cluster, int nlive, const double *vals,
                                     double *simplex, double *f)
{
    const int l0 = nT - 1;
    int ncl = 0, which = -1;
    for (int i = 0; i < nlive; ++i) ncl = std::max(ncl, cluster[i] + 1);
    double max_l = logzero;
    for (int c = 0; c < ncl; ++c) {
        std::vector<std::pair<double, int>> l;
        for (int i = 0; i < nlive; ++i)
            if (cluster[i] == c) l.push_back({ vals ? vals[i] : live[(size_t)i * nT + l0], i });
        if ((int)l.size() < D + 1) continue;
        std::stable_sort(l.begin(), l.end(), [](const std::pair<double, int> &a, const std::pair<double, int> &b) { return a.first < b.first; });
        if (l.back().first > max_l) {
            max_l = l.back().first;
            which = c;
            for (size_t k = l.size() - (D + 1), v = 0; k < l.size(); ++k, ++v) {
                std::copy(live + (size_t)l[k].second * nT, live + (size_t)l[k].second * nT + D, simplex + v * D);
                f[v] = l[k].first;
            }
        }
    }
    return max_l > logzero ? which : -1;
}

extern "C" void pc_maximum_alloc(pchip_maximum *m, int nDims, int nDerived)
{
    std::memset(m, 0, sizeof(*m));
    const size_t n = (size_t)(nDims + nDerived);
    m->max_point = (double *)std::calloc(n, sizeof(double));
    m->post_point = (double *)std::calloc(n, sizeof(double));
    m->mean_point = (double *)std::calloc(n, sizeof(double));
}

extern "C" void pchip_maximum_free(pchip_maximum *m)
{
    if (!m) return;
    std::free(m->max_point); std::free(m->post_point); std::free(m->mean_point);
    m->max_point = m->post_point = m->mean_point = nullptr;
}

// the values by the host functions: prior and loglikelihood callbacks, Nelder-Mead on the host
extern "C" int pchip_maximise_values(polychord_loglike_fn loglike, polychord_prior_fn prior, int nDims, int nDerived, double logzero,
                                     const double *live, const int *cluster, int nlive, const double *post_mean, pchip_maximum *out)
{
    const int D = nDims, nT = 2 * D + nDerived + 2, l0 = nT - 1;
    pc_maximum_alloc(out, D, nDerived);
    auto prior_of = [&](const double *cube, double *th) { prior(const_cast<double *>(cube), th, D); };
    auto dXdtheta = [&](const double *cube) {                             // maximiser.F90:179-207
        const double dx = 1e-5;
        std::vector<double> c0(D), t0(D), t1(D), J((size_t)D * D);
        prior_of(cube, t0.data());
        int s = 1;
        for (int i = 0; i < D; ++i) {
            std::copy(cube, cube + D, c0.begin());
            if (c0[i] + dx >= 1.0) { c0[i] -= dx; s = -s; } else c0[i] += dx;
            prior_of(c0.data(), t1.data());
            for (int r = 0; r < D; ++r) J[(size_t)i * D + r] = t1[r] - t0[r];
        }
        return D * std::log(dx) - std::log(s * det_cm(J, D));
    };
    auto point_of = [&](const double *cube, std::vector<double> &pt) {   // calculate_point (calculate.f90:6-50); true: the likelihood was called
        pt.assign(nT, 0.0);
        std::copy(cube, cube + D, pt.begin());
        bool inside = true;
        for (int d = 0; d < D; ++d) inside = inside && cube[d] >= 0.0 && cube[d] <= 1.0;
        if (!inside) { pt[l0] = logzero; return false; }
        prior_of(cube, pt.data() + D);
        pt[l0] = loglike(pt.data() + D, D, pt.data() + 2 * D, nDerived);
        return true;
    };
    auto maximisation = [&](int leg, std::vector<double> &best) -> bool {     // do_maximisation (maximiser.F90:92-161)
        std::vector<double> vals, simplex((size_t)(D + 1) * D), f(D + 1);
        if (leg == 1) {
            vals.resize(nlive);
            for (int i = 0; i < nlive; ++i) vals[i] = live[(size_t)i * nT + l0] + dXdtheta(live + (size_t)i * nT);
        }
        out->cluster[leg] = pc_max_choose_simplex(D, nT, logzero, live, cluster, nlive, leg == 1 ? vals.data() : nullptr, simplex.data(), f.data());
        if (out->cluster[leg] < 0) { std::printf("Could not construct simplex\n"); out->status[leg] = 1; return false; }
        std::vector<double> pt;
        auto func = [&](const double *x) {                                // maximisation_func (maximiser.F90:163-177)
            if (point_of(x, pt)) ++out->neval[leg];
            double v = pt[l0];
            if (leg == 1 && v > logzero) v += dXdtheta(x);
            return v;
        };
        const std::vector<double> x = nelder_mead(func, simplex, f, 1e-5, &out->niter[leg]);
        point_of(x.data(), best);
        return true;
    };
    std::vector<double> pmax, ppost;
    std::printf("-------------------------------------\nMaximising Likelihood\n");
    if (!maximisation(0, pmax)) { out->status[1] = 1; out->cluster[1] = -1; return 1; }
    std::printf("-------------------------------------\nMaximising Posterior\n");
    if (!maximisation(1, ppost)) return 1;
    const double dX = dXdtheta(ppost.data());
    out->max_logl = pmax[l0];
    std::copy(pmax.begin() + D, pmax.begin() + 2 * D + nDerived, out->max_point);
    out->max_post = ppost[l0] + dX;
    out->logl_at_post = ppost[l0];
    std::copy(ppost.begin() + D, ppost.begin() + 2 * D + nDerived, out->post_point);
    if (post_mean) {                                                       // maximiser.F90:77-80: likelihood at the posterior mean
        std::vector<double> mean(post_mean, post_mean + D + nDerived);
        out->has_mean = 1;
        out->logl_mean = loglike(mean.data(), D, mean.data() + D, nDerived);
        std::copy(mean.begin(), mean.end(), out->mean_point);
    }
    return 0;
}

// write_max_file (read_write.F90:754-807)
extern "C" int pchip_maximum_write(const pchip_maximum *m, int nDims, int nDerived, const char *path)
{
    const int D = nDims;
    if (!m || m->status[0] || m->status[1] || !m->max_point || !m->post_point) return 1;
    FILE *fo = std::fopen(path, "w");
    if (!fo) return 2;
    auto row = [&](const double *v, int n) { std::string s; for (int k = 0; k < n; ++k) s += e24(v[k]); std::fprintf(fo, "%s\n", s.c_str()); };
    std::fprintf(fo, "Maximum LogLikelihood:\n"); row(&m->max_logl, 1);
    std::fprintf(fo, "Maximum Likelihood point:\n"); row(m->max_point, D + nDerived); std::fprintf(fo, "\n");
    std::fprintf(fo, "Maximum Posterior:\n"); row(&m->max_post, 1);
    std::fprintf(fo, "Maximum Likelihood at posterior:\n"); row(&m->logl_at_post, 1);
    std::fprintf(fo, "Maximum Posterior point:\n"); row(m->post_point, D + nDerived); std::fprintf(fo, "\n");
    if (m->has_mean) {
        std::fprintf(fo, "LogLikelihood(mean):\n"); row(&m->logl_mean, 1);
        std::fprintf(fo, "mean point:\n"); row(m->mean_point, D + nDerived);
    }
    std::fclose(fo);
    return 0;
}

// live: [nlive][nTotal] rows [cube | theta | phi | birth | logL]; cluster: [nlive] labels; post_mean: [nDims + nDerived] or null
extern "C" int pchip_maximise(polychord_loglike_fn loglike, polychord_prior_fn prior, int nDims, int nDerived, double logzero,
                              const double *live, const int *cluster, int nlive, const double *post_mean, const char *path)
{
    pchip_maximum m;
    int rc = pchip_maximise_values(loglike, prior, nDims, nDerived, logzero, live, cluster, nlive, post_mean, &m);
    if (rc == 0) rc = pchip_maximum_write(&m, nDims, nDerived, path);
    pchip_maximum_free(&m);
    return rc;
}
