// pc_prior_table.h -- the prior table (pchip_prior.kind = PCHIP_PRIOR_TABLE) on the HOST: validation, the block structure the device
// kernels are given, and the ONE host implementation of the fifteen transforms (priors.f90:40-488, hypercube_to_physical :494-556) that
// polychord_hip_table_prior, the ini door, the engine's callback mode and the tests evaluate.  Host code only (not part of the run-time
// compiled kernel text); the device half is pc_table_theta in pc_sample.hip.
#pragma once
#include "../../include/polychord_hip.h"
#include <cmath>
#include <string>
#include <vector>

inline double pc_inv_normal_cdf_host(double p)
{   // Wichura AS241 PPND16 (utils.F90:806-966)
    static const double a[8] = { 3.3871328727963666080e+00, 1.3314166789178437745e+02, 1.9715909503065514427e+03, 1.3731693765509461125e+04, 4.5921953931549871457e+04, 6.7265770927008700853e+04, 3.3430575583588128105e+04, 2.5090809287301226727e+03 };
    static const double b[8] = { 1.0, 4.2313330701600911252e+01, 6.8718700749205790830e+02, 5.3941960214247511077e+03, 2.1213794301586595867e+04, 3.9307895800092710610e+04, 2.8729085735721942674e+04, 5.2264952788528545610e+03 };
    static const double c[8] = { 1.42343711074968357734e+00, 4.63033784615654529590e+00, 5.76949722146069140550e+00, 3.64784832476320460504e+00, 1.27045825245236838258e+00, 2.41780725177450611770e-01, 2.27238449892691845833e-02, 7.74545014278341407640e-04 };
    static const double d[8] = { 1.0, 2.05319162663775882187e+00, 1.67638483018380384940e+00, 6.89767334985100004550e-01, 1.48103976427480074590e-01, 1.51986665636164571966e-02, 5.47593808499534494600e-04, 1.05075007164441684324e-09 };
    static const double e[8] = { 6.65790464350110377720e+00, 5.46378491116411436990e+00, 1.78482653991729133580e+00, 2.96560571828504891230e-01, 2.65321895265761230930e-02, 1.24266094738807843860e-03, 2.71155556874348757815e-05, 2.01033439929228813265e-07 };
    static const double f[8] = { 1.0, 5.99832206555887937690e-01, 1.36929880922735805310e-01, 1.48753612908506148525e-02, 7.86869131145613259100e-04, 1.84631831751005468180e-05, 1.42151175831644588870e-07, 2.04426310338993978564e-15 };
    auto poly = [](const double *q, double x) { double v = 0; for (int i = 7; i >= 0; --i) v = v * x + q[i]; return v; };
    if (p <= 0) return -1.7976931348623157e308;
    if (p >= 1) return 1.7976931348623157e308;
    const double q = p - 0.5;
    if (std::fabs(q) <= 0.425) { const double r = 0.180625 - q * q; return q * poly(a, r) / poly(b, r); }
    double r = std::sqrt(-std::log(q < 0 ? p : 1 - p)), v;
    if (r <= 5) { r -= 1.6; v = poly(c, r) / poly(d, r); } else { r -= 5; v = poly(e, r) / poly(f, r); }
    return q < 0 ? -v : v;
}

// base type (1 .. 6) of a type number (1 .. 15), 0 for anything else; sorted_ forms 7 .. 10 and adaptive_sorted_ forms 11 .. 14 = uniform,
// gaussian, half_gaussian, exponential; nn_adaptive_layer_gaussian (15) = gaussian, which its layer coordinate turns into half_gaussian
inline int pc_prior_base_type(int type)
{
    if (type >= PCHIP_PT_UNIFORM && type <= PCHIP_PT_EXPONENTIAL) return type;
    switch (type) {
    case PCHIP_PT_SORTED_UNIFORM: case PCHIP_PT_ADAPTIVE_SORTED_UNIFORM: return PCHIP_PT_UNIFORM;
    case PCHIP_PT_SORTED_GAUSSIAN: case PCHIP_PT_ADAPTIVE_SORTED_GAUSSIAN: case PCHIP_PT_NN_ADAPTIVE_LAYER_GAUSSIAN: return PCHIP_PT_GAUSSIAN;
    case PCHIP_PT_SORTED_HALF_GAUSSIAN: case PCHIP_PT_ADAPTIVE_SORTED_HALF_GAUSSIAN: return PCHIP_PT_HALF_GAUSSIAN;
    case PCHIP_PT_SORTED_EXPONENTIAL: case PCHIP_PT_ADAPTIVE_SORTED_EXPONENTIAL: return PCHIP_PT_EXPONENTIAL;
    }
    return 0;
}
inline bool pc_prior_is_adaptive(int type) { return type >= PCHIP_PT_ADAPTIVE_SORTED_UNIFORM && type <= PCHIP_PT_NN_ADAPTIVE_LAYER_GAUSSIAN; }
inline int pc_prior_base_nparams(int base) { return base == PCHIP_PT_EXPONENTIAL ? 1 : (base == PCHIP_PT_POWER_UNIFORM ? 3 : 2); }
inline const char *pc_prior_type_name(int type)
{
    static const char *n[16] = { "?", "uniform", "log_uniform", "power_uniform", "gaussian", "half_gaussian", "exponential",
                                 "sorted_uniform", "sorted_gaussian", "sorted_half_gaussian", "sorted_exponential",
                                 "adaptive_sorted_uniform", "adaptive_sorted_gaussian", "adaptive_sorted_half_gaussian",
                                 "adaptive_sorted_exponential", "nn_adaptive_layer_gaussian" };
    return type >= 1 && type <= 15 ? n[type] : n[0];
}

// separable transforms of priors.f90:40-204 on one coordinate y in [0,1]
inline double pc_prior_base_transform(int base, double y, const double *pp)
{
    switch (base) {
    case PCHIP_PT_UNIFORM: return pp[0] + (pp[1] - pp[0]) * y;                                       // priors.f90:40-55
    case PCHIP_PT_LOG_UNIFORM: return pp[0] * std::pow(pp[1] / pp[0], y);                            // :114-128
    case PCHIP_PT_GAUSSIAN: return pp[0] + pp[1] * pc_inv_normal_cdf_host(y);                        // :73-88
    case PCHIP_PT_HALF_GAUSSIAN: return pp[0] + pp[1] * pc_inv_normal_cdf_host(0.5 + 0.5 * y);      // :172-187
    case PCHIP_PT_EXPONENTIAL: return -std::log(1.0 - y) / pp[0];                                    // :192-204
    default: {                                                                                       // power_uniform, :151-167
        const double a = std::pow(pp[0], 1.0 / pp[2]), b = std::pow(pp[1], 1.0 / pp[2]);
        return std::pow(a - y * std::fabs(a - b), pp[2]);
    }
    }
}

// x^(1/j) of a sorted_ block's member (priors.f90:245-262).  pow() of two libraries may differ in the last bit, and right below 1 that bit
// decides whether a block's largest member reaches the p >= 1 guard of AS241 (+huge) or stays at eight sigma.  So within 2^-33 of 1 the
// root is formed EXACTLY, the same way here and in the kernels (pc_table_theta): x = 1 - k 2^-53 with an integer k < 2^20, and
// (1 - k 2^-53)^(1/j) = 1 - (k / j) 2^-53 - O(k^2 2^-106) rounds to 1 - m 2^-53 with m = k / j rounded to nearest, a tie upwards (the
// second-order term breaks it; it is below 1 / (2 j) units for j <= 256) -- the correctly rounded value, which glibc's pow returns too
// except for the one tie j = 2, k = 1.  Elsewhere: pow.
inline double pc_sorted_root(double x, int j)
{
    if (x < 1.0 && x > 1.0 - 0x1p-33 && j <= 256) {
        const int k = (int)((1.0 - x) * 0x1p53);
        return 1.0 - (double)((2 * k + j) / (2 * j)) * 0x1p-53;
    }
    return std::pow(x, 1.0 / j);
}

// nfunc of an adaptive block of n parameters at its count coordinate x (priors.f90:378-380): INT(theta_1 + 0.5) with theta_1 = 0.5 + x (n - 1),
// every operation rounded on its own (no fma: the kernels form it with __dmul_rn / __dadd_rn), clamped to 1 .. n - 1 -- the reference
// comes out at n for x = 1 - 2^-53 and n - 1 a power of two, and sorts one element past its array there.
inline int pc_adaptive_nfunc(double x, int n)
{
    volatile double m = x * (double)(n - 1);
    volatile double t = 0.5 + m;
    volatile double u = t + 0.5;
    const int nf = (int)u;
    return nf < 1 ? 1 : (nf > n - 1 ? n - 1 : nf);
}
// the count's value, theta_1 (not rounded to an integer)
inline double pc_adaptive_count(double x, int n) { volatile double m = x * (double)(n - 1); return 0.5 + m; }

// the blocks of a table: sorted_ (7 .. 10) and adaptive (11 .. 15) types come as consecutive parameters of one type and block
// (priors.f90:245-262, :363-488; create_priors groups by type and block).  Fills pos / len / cnt / lay (see PcPriorTable); returns the first parameter
// found outside its block and that block's first parameter in (stray, head), or false.  The one block discovery: pc_prior_table_build and
// polychord_hip_ini_prior use it.
inline bool pc_prior_table_blocks(const std::vector<pchip_prior_entry> &e, std::vector<int> &pos, std::vector<int> &len, std::vector<int> &cnt,
                                  std::vector<int> &lay, int &stray, int &head)
{
    const int D = (int)e.size();
    pos.assign(D, 0); len.assign(D, 0); cnt.assign(D, -1); lay.assign(D, -1);
    stray = head = -1;
    for (int i = 0; i < D;) {
        if (e[i].type < PCHIP_PT_SORTED_UNIFORM) { ++i; continue; }
        int j = i;
        while (j < D && e[j].type == e[i].type && e[j].block == e[i].block) ++j;
        if (stray < 0)
            for (int k = j; k < D; ++k)
                if (e[k].type == e[i].type && e[k].block == e[i].block) { stray = k; head = i; break; }
        if (!pc_prior_is_adaptive(e[i].type)) {
            for (int k = i; k < j; ++k) { pos[k] = k - i + 1; len[k] = j - i; }
        } else {
            // the count is the block's first parameter -- behind the layer parameter in type 15 --, the members follow it: pos counts them from 1,
            // len is their number (the largest nfunc)
            const int c = i + (e[i].type == PCHIP_PT_NN_ADAPTIVE_LAYER_GAUSSIAN ? 1 : 0);
            for (int k = c + 1; k < j; ++k) { pos[k] = k - c; len[k] = j - c - 1; cnt[k] = c; if (c > i) lay[k] = i; }
        }
        i = j;
    }
    return stray >= 0;
}

struct PcPriorTable {
    int D = 0;
    std::vector<pchip_prior_entry> e;      // [D] in PARAMETER order
    std::vector<int> hyper;                // [D] hypercube index of every parameter (priors.f90:708-737)
    std::vector<int> pos, len;             // [D] sorted_ blocks: 1-based position in the block and its length; 0, 0 elsewhere
    //   the members of an adaptive block (the parameters behind its count): 1-based position among them and their number
    std::vector<int> cnt, lay;             // [D] a member of an adaptive block: PARAMETER index of its count and, type 15, of its layer; -1 elsewhere
    unsigned mask = 0;                     // bit t: base type t is present; bit 16: a sorted_ or adaptive block; bit 17: the order is no identity;
    //   bit 18: an adaptive block (types 11 .. 15); bit 19: a layer parameter (type 15)
    bool is_box = false;                   // all uniform, identity order: the engine runs it as the uniform box
    bool is_count(int i) const { return pc_prior_is_adaptive(e[i].type) && pos[i] == 0; }      // a count or layer parameter
    // what the device kernels read (pc_table_theta): doubles [3][D], integers [6][D] = base type, pos, len, hyper, and the HYPERCUBE index
    // of the count's and of the layer's coordinate of a member of an adaptive block (-1 elsewhere): what such a lane reads of the staged cube
    // (per base type, the constants of the host formulas above formed HERE, with the host's pow: uniform lo, hi - lo; log_uniform lo, hi / lo;
    //  power_uniform a = lo^(1/p), |a - hi^(1/p)|, p; gaussian / half_gaussian mu, sigma; exponential the rate.  The count of an adaptive
    //  block of n is a uniform entry with lo 0.5 and span n - 1, the layer of type 15 one with span 2.)
    std::vector<double> dev_par() const
    {
        std::vector<double> v((size_t)3 * D, 0.0);
        for (int i = 0; i < D; ++i) {
            const double *pp = e[i].par;
            double c[3] = { pp[0], 0.0, 0.0 };
            if (is_count(i)) { c[0] = 0.5; c[1] = count_span(i); for (int k = 0; k < 3; ++k) v[(size_t)k * D + i] = c[k]; continue; }
            switch (pc_prior_base_type(e[i].type)) {
            case PCHIP_PT_UNIFORM: c[1] = pp[1] - pp[0]; break;
            case PCHIP_PT_LOG_UNIFORM: c[1] = pp[1] / pp[0]; break;
            case PCHIP_PT_POWER_UNIFORM: { const double a = std::pow(pp[0], 1.0 / pp[2]), b = std::pow(pp[1], 1.0 / pp[2]); c[0] = a; c[1] = std::fabs(a - b); c[2] = pp[2]; break; }
            case PCHIP_PT_EXPONENTIAL: break;
            default: c[1] = pp[1]; break;
            }
            for (int k = 0; k < 3; ++k) v[(size_t)k * D + i] = c[k];
        }
        return v;
    }
    std::vector<int> dev_int() const
    {
        std::vector<int> v((size_t)6 * D);
        for (int i = 0; i < D; ++i) {
            v[i] = is_count(i) ? PCHIP_PT_UNIFORM : pc_prior_base_type(e[i].type);
            v[(size_t)D + i] = pos[i]; v[(size_t)2 * D + i] = len[i]; v[(size_t)3 * D + i] = hyper[i]; v[(size_t)4 * D + i] = cnt[i] >= 0 ? hyper[cnt[i]] : -1; v[(size_t)5 * D + i] = lay[i] >= 0 ? hyper[lay[i]] : -1;
        }
        return v;
    }
    // span of a count or layer parameter's uniform value on top of 0.5: the layer 2, a count the number of its members
    bool is_layer(int i) const { return i + 2 < D && lay[i + 2] == i; }                         // (the first member lies two behind its layer)
    double count_span(int i) const
    {
        if (is_layer(i)) return 2.0;
        return i + 1 < D && cnt[i + 1] == i ? (double)len[i + 1] : 0.0;
    }
};

// checks a table and derives the block structure; returns "" or the message (which names the parameter, 1-based like the ini file's lines)
inline std::string pc_prior_table_build(int D, const pchip_prior_entry *entries, const int *hyper, PcPriorTable &T)
{
    if (D < 1 || !entries) return "a prior table needs nDims >= 1 entries";
    T = PcPriorTable();
    T.D = D; T.e.assign(entries, entries + D); T.hyper.resize(D); T.pos.assign(D, 0); T.len.assign(D, 0);
    auto par = [](int i) { return "parameter " + std::to_string(i + 1); };
    std::vector<char> seen((size_t)D, 0);
    bool identity = true, all_uniform = true, adaptive = false;
    for (int i = 0; i < D; ++i) {
        const int h = hyper ? hyper[i] : i;
        if (h < 0 || h >= D || seen[h]) return "prior table: the hypercube order is no permutation of 0 .. nDims-1 (" + par(i) + ": index " + std::to_string(h) + ")";
        seen[h] = 1; T.hyper[i] = h; identity = identity && h == i;
    }
    for (int i = 0; i < D; ++i) {
        const pchip_prior_entry &p = T.e[i];
        const int base = pc_prior_base_type(p.type);
        if (!base) return "prior table: unknown prior type " + std::to_string(p.type) + " for " + par(i) + " (types 1 .. 15)";
        const int need = pc_prior_base_nparams(base);
        if (pc_prior_is_adaptive(p.type)) {
            // the reference skips the count's (and the layer's) prior parameters by position (priors.f90:401, :458, :483): every parameter of the block
            // gives exactly the base type's number; a count's and a layer's values are read and ignored
            if (p.npar != need) return "prior table: " + par(i) + " (" + pc_prior_type_name(p.type) + ") needs exactly " + std::to_string(need) + " prior parameters, not " + std::to_string(p.npar);
            adaptive = true; all_uniform = false;
            continue;                          // (values and mask: below, once the blocks tell members from counts)
        }
        if (p.npar < need) return "prior table: " + par(i) + " (" + pc_prior_type_name(p.type) + ") needs " + std::to_string(need) + " prior parameters, not " + std::to_string(p.npar);
        if (p.npar > 3) return "prior table: " + par(i) + " has " + std::to_string(p.npar) + " prior parameters: at most 3";
        for (int k = 0; k < need; ++k) if (!std::isfinite(p.par[k])) return "prior table: " + par(i) + " has a prior parameter that is not finite";
        if (base == PCHIP_PT_LOG_UNIFORM && !(p.par[0] > 0.0 && p.par[1] > 0.0)) return "prior table: " + par(i) + " (log_uniform) needs positive bounds";
        if (base == PCHIP_PT_POWER_UNIFORM && (!(p.par[0] > 0.0 && p.par[1] > 0.0) || p.par[2] == 0.0)) return "prior table: " + par(i) + " (power_uniform) needs positive bounds and a power that is not zero";
        if ((base == PCHIP_PT_GAUSSIAN || base == PCHIP_PT_HALF_GAUSSIAN) && !(p.par[1] > 0.0)) return "prior table: " + par(i) + " (" + pc_prior_type_name(p.type) + ") needs sigma > 0";
        if (base == PCHIP_PT_EXPONENTIAL && !(p.par[0] > 0.0)) return "prior table: " + par(i) + " (" + pc_prior_type_name(p.type) + ") needs a rate > 0";
        all_uniform = all_uniform && p.type == PCHIP_PT_UNIFORM;
        T.mask |= 1u << base;
    }
    // sorted_ and adaptive blocks: consecutive parameters of one type and block
    int stray, head;
    if (pc_prior_table_blocks(T.e, T.pos, T.len, T.cnt, T.lay, stray, head))
        return "prior table: the members of a sorted block must be consecutive parameters of one type and block (" + par(stray) + " belongs to the block of " + par(head) + ")";
    for (int i = 0; i < D; ++i) if (T.len[i] > 0) T.mask |= 1u << 16;
    if (adaptive) {
        for (int i = 0; i < D;) {
            const pchip_prior_entry &p = T.e[i];
            if (!pc_prior_is_adaptive(p.type)) { ++i; continue; }
            int j = i;
            while (j < D && T.e[j].type == p.type && T.e[j].block == p.block) ++j;
            const bool nn = p.type == PCHIP_PT_NN_ADAPTIVE_LAYER_GAUSSIAN;
            // a block without a member has no meaning in the reference either (it sorts outside its array); to a caller who meant something
            // else by the number, it is an unknown prior type
            if (j - i < (nn ? 3 : 2))
                return "prior table: " + par(i) + ": a block of " + std::to_string(j - i) + " is an unknown prior type " + std::to_string(p.type) + " (" + pc_prior_type_name(p.type) +
                       " needs " + (nn ? "its layer, its count and at least one member: 3" : "its count and at least one member: 2") + " consecutive parameters of one block)";
            if (j - i - (nn ? 2 : 1) > 256) return "prior table: " + par(i) + ": an adaptive block has at most 256 members";
            const int base = pc_prior_base_type(p.type);
            for (int k = i + (nn ? 2 : 1); k < j; ++k) {
                const pchip_prior_entry &q = T.e[k];
                for (int m = 0; m < q.npar; ++m) if (!std::isfinite(q.par[m])) return "prior table: " + par(k) + " has a prior parameter that is not finite";
                if ((base == PCHIP_PT_GAUSSIAN || base == PCHIP_PT_HALF_GAUSSIAN) && !(q.par[1] > 0.0)) return "prior table: " + par(k) + " (" + pc_prior_type_name(q.type) + ") needs sigma > 0";
                if (base == PCHIP_PT_EXPONENTIAL && !(q.par[0] > 0.0)) return "prior table: " + par(k) + " (" + pc_prior_type_name(q.type) + ") needs a rate > 0";
            }
            T.mask |= (1u << PCHIP_PT_UNIFORM) | (1u << base) | (1u << 18);
            if (nn) T.mask |= (1u << PCHIP_PT_HALF_GAUSSIAN) | (1u << 19);
            i = j;
        }
    }
    if (!identity) T.mask |= 1u << 17;
    T.is_box = all_uniform && identity;
    return "";
}

// hypercube_to_physical (priors.f90:494-556): separable blocks, and sorted_ blocks = the order statistics of the block's coordinates
// (priors.f90:245-262: y_n = x_n^(1/n), y_k = y_{k+1} x_k^(1/k)) pushed through the separable transform.  Adaptive blocks (:363-488): the
// count's coordinate decides how many of the members are order statistics (the first nfunc; the others keep y = x), and the layer's
// coordinate of type 15 whether the members' base is half_gaussian (theta_1 < 1.5) or gaussian.
inline void pc_prior_table_eval(const PcPriorTable &T, const double *cube_h, double *theta)
{
    const int D = T.D;
    for (int i = 0; i < D;) {
        int base = pc_prior_base_type(T.e[i].type);
        if (pc_prior_is_adaptive(T.e[i].type)) {
            if (T.pos[i] == 0) {               // the layer (span 2: 0.5 + 2 x is exact up to its one rounding) or the count
                theta[i] = T.is_layer(i) ? 0.5 + cube_h[T.hyper[i]] * 2.0 : pc_adaptive_count(cube_h[T.hyper[i]], (int)T.count_span(i) + 1);
                ++i;
                continue;
            }
            const int n = T.len[i], nfunc = pc_adaptive_nfunc(cube_h[T.hyper[T.cnt[i]]], n + 1);
            if (T.lay[i] >= 0 && 0.5 + cube_h[T.hyper[T.lay[i]]] * 2.0 < 1.5) base = PCHIP_PT_HALF_GAUSSIAN;
            double prev = 1.0;
            for (int k = n; k >= 1; --k) {
                double y = cube_h[T.hyper[i + k - 1]];
                if (k <= nfunc) y = prev = prev * pc_sorted_root(y, k);
                theta[i + k - 1] = pc_prior_base_transform(base, y, T.e[i + k - 1].par);
            }
            i += n;
            continue;
        }
        if (T.len[i] > 0) {
            const int n = T.len[i];
            double prev = 1.0;
            for (int k = n; k >= 1; --k) {
                prev = prev * pc_sorted_root(cube_h[T.hyper[i + k - 1]], k);
                theta[i + k - 1] = pc_prior_base_transform(base, prev, T.e[i + k - 1].par);
            }
            i += n;
            continue;
        }
        theta[i] = pc_prior_base_transform(base, cube_h[T.hyper[i]], T.e[i].par);
        ++i;
    }
}
