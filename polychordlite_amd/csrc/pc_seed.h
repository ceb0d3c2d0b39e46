// pc_seed.h -- what the direction kernels (pc_bases.hip) and the slice-sampling chains (pc_sample.hip, pc_slice_body.inc) share: the choice
// of a chain's seed point (GenerateSeed, generate.F90:19-55), by one thread or by a wavefront, and the chain's deck -- its shuffle, its tag and
// where its record lies behind the bases.  Device code only; part of the text that pc_rtc.hip compiles at run time, because k_slice uses it.
#pragma once
#include "pc_state.h"

__device__ __forceinline__ void select_seed(const PcState &S, unsigned batch, int chain, int &sel, int &slot)
{   // GenerateSeed, generate.F90:42-53; random_integer_P random_utils.F90:548-576
    const int nc = S.ctl->ncluster;
    if (nc == 1) {       // one cluster: the volume-weighted draw (generate.F90:36-41) can only return it
        sel = 0;
        const double u2s = S.seq_mode ? pc_seq_uniform(S, S.ctl->seq + 1) : pc_uniform(S.k0, S.k1, PC_DOM_SEED, batch, (uint32_t)chain, 1u);
        const int ns = S.cl_n[0];
        int is = (int)ceil(u2s * ns);
        is = is < 1 ? 1 : (is > ns ? ns : is);
        slot = S.cl_list[is - 1];
        if (S.seed_override) slot = chain;
        return;
    }
    double m = S.logXp[0];
    for (int c = 1; c < nc; ++c) m = fmax(m, S.logXp[c]);
    double sum = 0.0;
    for (int c = 0; c < nc; ++c) sum += exp(S.logXp[c] - m);
    const double lse = m + log(sum);
    double norm = 0.0;
    for (int c = 0; c < nc; ++c) norm += exp(S.logXp[c] - lse);
    const double u = S.seq_mode ? pc_seq_uniform(S, S.ctl->seq) : pc_uniform(S.k0, S.k1, PC_DOM_SEED, batch, (uint32_t)chain, 0u);
    double cdf = 0.0;
    sel = nc - 1;
    for (int c = 0; c < nc; ++c) { cdf += exp(S.logXp[c] - lse) / norm; if (u < cdf) { sel = c; break; } }
    const double u2 = S.seq_mode ? pc_seq_uniform(S, S.ctl->seq + 1) : pc_uniform(S.k0, S.k1, PC_DOM_SEED, batch, (uint32_t)chain, 1u);
    const int n = S.cl_n[sel];
    int idx = (int)ceil(u2 * n);
    idx = idx < 1 ? 1 : (idx > n ? n : idx);
    slot = S.cl_list[(size_t)sel * S.Ncap + idx - 1];
    if (S.seed_override) slot = chain;
}

// The deck of a chain (chordal_sampling.f90:135-142, random_utils.F90:505-532: the first direction stays, the others are Fisher-Yates shuffled),
// num_repeats <= 64: the value for position p lives in lane p.  With keyed draws a pure function of (keys, nursery, chain): k_slice makes it, or finds
// it behind the bases where k_nhats<.., 1> / k_nhats_w (pc_bases.hip) left it on the side stream under a tag of those four numbers -- a matching
// tag IS the right deck, whatever older run wrote it.  So the writers' deck and k_slice's own must be the same bits, or a run's numbers would
// depend on whether a record happened to be there: ONE text, PC_DECK_SHUFFLE, declares the deck `dk` of this lane.  SEQ: the draws come from
// the sequential stream (k_slice's rare mode, never a record), draw of position p at seq_g0 + nr - 1 - p; false: keyed.
// Text, not a function, as PC_GS_PACKED of pc_dev.h is: inlined from a __forceinline__ function the same statements reach the register
// allocator in another order, and eight of the default k_slice variants would no longer be the instructions they were (tools/dev/isa_diff.py).
#define PC_DECK_SHUFFLE(dk, S, batch, chain, lane, nr, SEQ, seq_g0) \
    int dk = lane, jv = 0; \
    if (lane >= 1 && lane < nr) { \
        const double u = (SEQ) ? pc_seq_uniform(S, (seq_g0) + (unsigned long long)(nr - 1 - lane)) \
                               : pc_uniform(S.k0, S.k1, PC_DOM_SHUFFLE, batch, (uint32_t)chain, (uint32_t)lane); \
        int j = (int)ceil(u * lane); \
        jv = j < 1 ? 1 : (j > lane ? lane : j); \
    } \
    for (int i = nr - 1; i >= 1; --i) { \
        const int j = __builtin_amdgcn_readlane(jv, i); \
        const int di = __builtin_amdgcn_readlane(dk, i), dj = __builtin_amdgcn_readlane(dk, j); \
        dk = (lane == i) ? dj : ((lane == j) ? di : dk); \
    }
// the keyed deck, as the writers of a record make it
__device__ __forceinline__ int pc_deck_keyed(const PcState &S, unsigned batch, int chain, int lane, int nr)
{
    PC_DECK_SHUFFLE(dk, S, batch, chain, lane, nr, false, 0ull)
    return dk;
}
// (everything the deck is a function of; a record that carries this tag carries that deck, whichever run, shape or buffer layout wrote it)
__device__ __forceinline__ unsigned long long pc_deck_tag(const PcState &S, unsigned batch, int chain, int nr)
{
    return ((((unsigned long long)S.k0 << 32) | (unsigned long long)S.k1) ^ ((unsigned long long)batch * 0x9E3779B97F4A7C15ull)
            ^ ((unsigned long long)(unsigned)chain * 0xC2B2AE3D27D4EB4Full) ^ ((unsigned long long)(unsigned)nr << 56)) | 1ull;
}
// behind the bases of a nursery (nDims <= 24: the engine allocates the tail): one record of 66 ints a chain, [tag lo, tag hi, deck[64]]
__device__ __forceinline__ int *pc_deck_record(const PcState &S, int chain) { return (int *)(S.nhat_raw + (size_t)S.B * S.nb_total * S.D * S.D) + (size_t)chain * 66; }

// select_seed by a whole wavefront (several clusters): the same numbers -- every exponential and quotient has the operands of the loops above and
// every sum their order -- with the clusters' volumes loaded and exponentiated a lane each and only the additions in sequence (v_readlane): one
// thread's three loops of a dependent global load + exponential per cluster were ~30 k cycles in front of every chain at two dozen clusters.
__device__ __forceinline__ void select_seed_wave(const PcState &S, unsigned batch, int chain, int lane, int &sel, int &slot)
{
    const int nc = S.ctl->ncluster;
    if (nc == 1 || S.seq_mode) {
        int a = 0, b = 0;
        if (lane == 0) select_seed(S, batch, chain, a, b);
        sel = __builtin_amdgcn_readfirstlane(a); slot = __builtin_amdgcn_readfirstlane(b);
        return;
    }
    double m = -PC_HUGE;
    for (int c0 = 0; c0 < nc; c0 += 64) { const int c = c0 + lane; m = fmax(m, c < nc ? S.logXp[c] : -PC_HUGE); }
    m = wave_max(m);
    double sum = 0.0;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        const double e = c < nc ? exp(S.logXp[c] - m) : 0.0;
        const int n = nc - c0 < 64 ? nc - c0 : 64;
        for (int q = 0; q < n; ++q) sum += readlane_f64(e, q);
    }
    const double lse = m + log(sum);
    double norm = 0.0;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        const double t = c < nc ? exp(S.logXp[c] - lse) : 0.0;
        const int n = nc - c0 < 64 ? nc - c0 : 64;
        for (int q = 0; q < n; ++q) norm += readlane_f64(t, q);
    }
    const double u = pc_uniform(S.k0, S.k1, PC_DOM_SEED, batch, (uint32_t)chain, 0u);
    double cdf = 0.0;
    sel = nc - 1;
    bool found = false;
    for (int c0 = 0; c0 < nc && !found; c0 += 64) {
        const int c = c0 + lane;
        const double r = c < nc ? exp(S.logXp[c] - lse) / norm : 0.0;
        const int n = nc - c0 < 64 ? nc - c0 : 64;
        for (int q = 0; q < n; ++q) { cdf += readlane_f64(r, q); if (u < cdf) { sel = c0 + q; found = true; break; } }
    }
    const double u2 = pc_uniform(S.k0, S.k1, PC_DOM_SEED, batch, (uint32_t)chain, 1u);
    const int n = S.cl_n[sel];
    int idx = (int)ceil(u2 * n);
    idx = idx < 1 ? 1 : (idx > n ? n : idx);
    slot = S.cl_list[(size_t)sel * S.Ncap + idx - 1];
    if (S.seed_override) slot = chain;
}

