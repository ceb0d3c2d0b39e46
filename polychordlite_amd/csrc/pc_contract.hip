// pc_contract.hip -- nested-sampling contraction on the device: the general serial kernel and the candidate lists in front of it.
//
//   k_consume   ONE workgroup walks the nursery in the reference's order and takes every decision
//               of replace_point / delete_outermost_point / update_evidence / find_min_loglikelihoods /
//               more_samples_needed / delete_cluster (run_time_info.f90:716-817, 211-296, 883-909,
//               507-598; nested_sampling.F90:239-341, 514-543).  The live logL column and the
//               (cluster, list position) labels of every slot sit in LDS; the independent log-space
//               updates of one death are spread over lanes; min-logL scans are DPP argmin butterflies.
//               No point row is moved here: the kernel emits a PLAN.
//   k_nn_lists* / k_nn_gather* / k_nn_lists_d<D>*   the candidate lists of identify_cluster, made in front of it.
//   k_init_state   the initial per-cluster state and control block.
// The row kernels that execute the plan (k_apply_*, k_install_live) are pc_rows.hip; the "update" step taken kernel by kernel
// (k_clean_* / k_cov_* / k_chol*) is pc_update_steps.hip.
#include "pc_state.h"
#include "pc_launch.h"
#include "pc_block.h"
#include <atomic>
#include <cstdlib>
#include <type_traits>

struct ConsumeShared {
    double *sL; int *sC; int *sP;                      // per slot
    double *cLogLp, *cLogXp, *cLogZp, *cLogZXp, *cLogZp2, *cLogZpXp, *cLseRef, *cLseSum, *cThr;
    int *cN, *cMinSlot; unsigned *cUid;
    double *jobres;                                     // [NT] results of the lane-parallel jobs
    vk_t *red;                                          // [16]
    double *xbuf;                                       // [IDG][D] cube coordinates of the babies being identified
    double *sX;                                         // [xrows][D] cube coordinates: all live points (xrows == Ncap) or one tile
    int xrows;
    double *gd2; int *gkey; int *ids;                   // [IDG][IDP] partial minima; [nr] cluster of each baby
    int *misc;                                          // small scratch
    int *sO, *sCS;                                      // nn_slot_owner [Ncap], nn_chain_slot [B] (only when S.nn_valid)
    double *xq; int xq_ld;                              // log <X_p X_q>: LDS copy [xq_ld][xq_ld] when the clusters fit, else S.XpXq [maxc][maxc]
};

// identify_cluster (run_time_info.f90:913-949) for ALL babies of a chain at once: the cluster of the
// nearest live point over all clusters; ties keep the first point in (cluster, list position) order
// like the reference's strict '<' scan.  Babies are taken in groups of IDG; inside a group IDP = NT/IDG
// threads share one baby, each scanning a stride of the live slots; the live coordinates are served
// from the LDS cache H.sX when it fits (updated on every insertion), else from HBM.
#define PC_IDG 32
template <int NT>
__device__ void block_identify_all(const PcState &S, const ConsumeShared &H, int w, const double *blog, double Lg, int nc,
                                   bool only_unresolved = false)
{
    const int tid = threadIdx.x, D = S.D, nr = S.nr, nT = S.nT;
    constexpr int IDG = (NT >= 1024) ? PC_IDG : 4, IDP = NT / IDG;
    if (!only_unresolved) for (int i = tid; i < nr; i += NT) H.ids[i] = -1;
    if (nc == 1) { __syncthreads(); for (int i = tid; i < nr; i += NT) H.ids[i] = 0; __syncthreads(); return; }
    for (int g0 = 0; g0 < nr; g0 += IDG) {
        __syncthreads();
        if (only_unresolved) {                          // skip groups that the candidate lists settled completely
            bool need = false;
            for (int g = 0; g < IDG && g0 + g < nr; ++g) need = need || (H.ids[g0 + g] == -2);
            if (!need) continue;
        }
        for (int e = tid; e < IDG * D; e += NT) {
            const int g = e / D, d = e % D, i = g0 + g;
            H.xbuf[e] = (i < nr) ? S.babies[((size_t)w * nr + i) * nT + d] : 0.0;
        }
        __syncthreads();
        const int g = tid / IDP, p = tid % IDP, i = g0 + g;
        double bd = PC_HUGE; int bk = 0x7fffffff;
        const bool mine = i < nr && blog[i] > Lg && (!only_unresolved || H.ids[i] == -2);
        const double *x = H.xbuf + (size_t)g * D;
        if (H.xrows >= S.Ncap) {                       // every live coordinate is resident in LDS
            if (mine)
                for (int s = p; s < S.Ncap; s += IDP) {
                    const int c = H.sC[s];
                    if (c < 0) continue;
                    const double *q = H.sX + (size_t)s * D;
                    double d2 = 0.0;
                    for (int d = 0; d < D; ++d) { const double t = x[d] - q[d]; d2 += t * t; }
                    const int key = c * S.Ncap + H.sP[s];
                    if (d2 < bd || (d2 == bd && key < bk)) { bd = d2; bk = key; }
                }
        } else {                                       // stream the live coordinates through an LDS tile
            for (int t0 = 0; t0 < S.Ncap; t0 += H.xrows) {
                const int tn = min(H.xrows, S.Ncap - t0);
                __syncthreads();
                for (int e = tid; e < tn * D; e += NT) {
                    const int s = t0 + e / D, d = e % D, src = S.slot_src[s];
                    H.sX[e] = (src >= 0) ? S.babies[((size_t)src * nr + (nr - 1)) * nT + d] : S.live[(size_t)s * nT + d];
                }
                __syncthreads();
                if (mine)
                    for (int sl = p; sl < tn; sl += IDP) {
                        const int s = t0 + sl, c = H.sC[s];
                        if (c < 0) continue;
                        const double *q = H.sX + (size_t)sl * D;
                        double d2 = 0.0;
                        for (int d = 0; d < D; ++d) { const double t = x[d] - q[d]; d2 += t * t; }
                        const int key = c * S.Ncap + H.sP[s];
                        if (d2 < bd || (d2 == bd && key < bk)) { bd = d2; bk = key; }
                    }
            }
        }
        H.gd2[tid] = bd; H.gkey[tid] = bk;
        __syncthreads();
        if (tid < IDG && g0 + tid < nr && (!only_unresolved || H.ids[g0 + tid] == -2)) {
            double md = PC_HUGE; int mk = 0x7fffffff;
            for (int q = 0; q < IDP; ++q) {
                const double v = H.gd2[tid * IDP + q]; const int k = H.gkey[tid * IDP + q];
                if (v < md || (v == md && k < mk)) { md = v; mk = k; }
            }
            H.ids[g0 + tid] = (mk == 0x7fffffff) ? -1 : mk / S.Ncap;
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// k_nn_lists: the nearest-cluster search of a whole nursery, done once by the whole chip.
//
// identify_cluster (run_time_info.f90:913-949) asks, for every baby, for the nearest live point AT THE MOMENT ITS
// CHAIN IS CONSUMED; between the consumption of two chains the live set changes by one point, so the reference's
// answer is a property of an evolving set and the serial contraction used to recompute N x D distances per baby on one
// CU.  But every point that can be alive then is known now (T0): the live points of T0 and the last babies of the
// chains consumed before this one (reverse nursery order: chains w' > w).  One workgroup per unconsumed chain ranks
// that superset for each of its babies and keeps the PC_NN_K nearest, ascending; the contraction then only walks the
// list for the first entry that is still / already alive (exact: everything nearer is dead), and falls back to the
// full search when a list is exhausted.
//   256 threads = 32 babies x 8 partial scanners; points are staged through an LDS tile.
// ------------------------------------------------------------------------------------------
#define NNL_G 32
#define NNL_P 8
__device__ __forceinline__ void nn_lists_body(const PcState &S, int nleft, int tile_pts)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, D = S.D, nr = S.nr, nT = S.nT, Ncap = S.Ncap;
    const int w = blockIdx.x;                         // chain, w < nleft = entries still in the nursery
    double *xb = (double *)smem;                      // [NNL_G][D] babies of the group
    double *pts = xb + (size_t)NNL_G * D;             // [tile_pts][D]
    double *md = pts + (size_t)tile_pts * D;          // [256][PC_NN_K] merge buffer
    int *mc = (int *)(md + 256 * PC_NN_K);            // [256][PC_NN_K]
    int *pcode = mc + 256 * PC_NN_K;                  // [tile_pts] code of each staged point, PC_NN_NONE = skip
    if (w == 0) {                                     // liveness bookkeeping starts now
        for (int s = tid; s < Ncap; s += 256) S.nn_slot_owner[s] = -1;
        for (int c = tid; c < S.B; c += 256) S.nn_chain_slot[c] = -1;
    }
    const int nc = S.ctl->ncluster;
    double Lg0 = S.logLp[0];
    for (int c = 1; c < nc; ++c) Lg0 = fmin(Lg0, S.logLp[c]);
    const double *blog = S.baby_logL + (size_t)w * nr;
    const int ncand = nleft - 1 - w;                  // chains w+1 .. nleft-1 are consumed before w
    const int npts = Ncap + ncand;
    const int g = tid / NNL_P, p = tid % NNL_P;
    for (int g0 = 0; g0 < nr; g0 += NNL_G) {
        __syncthreads();
        for (int e = tid; e < NNL_G * D; e += 256) {
            const int gg = e / D, d = e % D, i = g0 + gg;
            xb[e] = (i < nr) ? S.babies[((size_t)w * nr + i) * nT + d] : 0.0;
        }
        const int i = g0 + g;
        const bool mine = i < nr && blog[i] > Lg0;    // the contour only rises: others never need a cluster
        double bd[PC_NN_K]; int bc[PC_NN_K];
#pragma unroll
        for (int k = 0; k < PC_NN_K; ++k) { bd[k] = PC_HUGE; bc[k] = PC_NN_NONE; }
        for (int t0 = 0; t0 < npts; t0 += tile_pts) {
            const int tn = min(tile_pts, npts - t0);
            __syncthreads();
            for (int q = tid; q < tn; q += 256) {
                const int gi = t0 + q;
                int code = PC_NN_NONE;
                if (gi < Ncap) { if (S.live_cluster[gi] >= 0) code = gi; }
                else code = -(1 + (w + 1 + (gi - Ncap)));
                pcode[q] = code;
            }
            __syncthreads();
            for (int e = tid; e < tn * D; e += 256) {
                const int q = e / D, d = e % D, code = pcode[q];
                double v = 0.0;
                if (code >= 0) { const int src = S.slot_src[code]; v = (src >= 0) ? S.babies[((size_t)src * nr + (nr - 1)) * nT + d] : S.live[(size_t)code * nT + d]; }
                else if (code != PC_NN_NONE) v = S.babies[((size_t)(-(1 + code)) * nr + (nr - 1)) * nT + d];
                pts[e] = v;
            }
            __syncthreads();
            if (mine) {
                const double *x = xb + (size_t)g * D;
                for (int q = p; q < tn; q += NNL_P) {
                    const int code = pcode[q];
                    if (code == PC_NN_NONE) continue;
                    const double *y = pts + (size_t)q * D;
                    double d2 = 0.0;
                    for (int d = 0; d < D; ++d) { const double t = x[d] - y[d]; d2 += t * t; }
                    if (d2 < bd[PC_NN_K - 1]) {       // sorted insertion, registers only
                        double cd = d2; int cc = code;
#pragma unroll
                        for (int k = 0; k < PC_NN_K; ++k) {
                            const bool sw = cd < bd[k];
                            const double td = sw ? bd[k] : cd; const int tc = sw ? bc[k] : cc;
                            bd[k] = sw ? cd : bd[k]; bc[k] = sw ? cc : bc[k];
                            cd = td; cc = tc;
                        }
                    }
                }
            }
        }
        // merge the NNL_P partial lists of a baby: each is sorted, NNL_P-way pick by the first scanner
#pragma unroll
        for (int k = 0; k < PC_NN_K; ++k) { md[tid * PC_NN_K + k] = bd[k]; mc[tid * PC_NN_K + k] = bc[k]; }
        __syncthreads();
        if (p == 0 && i < nr) {
            int head[NNL_P];
#pragma unroll
            for (int q = 0; q < NNL_P; ++q) head[q] = 0;
            int out[PC_NN_K];
#pragma unroll
            for (int k = 0; k < PC_NN_K; ++k) {
                double best = PC_HUGE; int bq = -1;
#pragma unroll
                for (int q = 0; q < NNL_P; ++q) {
                    const double v = (head[q] < PC_NN_K) ? md[(g * NNL_P + q) * PC_NN_K + head[q]] : PC_HUGE;
                    if (v < best) { best = v; bq = q; }
                }
                int code = PC_NN_NONE;
#pragma unroll
                for (int q = 0; q < NNL_P; ++q) if (q == bq) { code = mc[(g * NNL_P + q) * PC_NN_K + head[q]]; head[q]++; }
                out[k] = mine ? code : PC_NN_NONE;
            }
            int4 *dst = (int4 *)(S.nn_list + ((size_t)w * nr + i) * PC_NN_K);
            dst[0] = make_int4(out[0], out[1], out[2], out[3]);
            dst[1] = make_int4(out[4], out[5], out[6], out[7]);
        }
    }
}
__global__ __launch_bounds__(256) void k_nn_lists(PcState S, int nleft, int tile_pts) { nn_lists_body(S, nleft, tile_pts); }
// several runs in step (blockIdx.y = run): each run its own number of chains left in the nursery (PcManyRec::ia[PC_REC_I_NLEFT])
__global__ __launch_bounds__(256) void k_nn_lists_many(const PcManyRec *__restrict__ R, int tile_pts)
{
    const PcManyView r = pc_many_view(R, blockIdx.y);
    if ((int)blockIdx.x >= r.ia[PC_REC_I_NLEFT]) return;
    nn_lists_body(r.S, r.ia[PC_REC_I_NLEFT], tile_pts);
}

// ------------------------------------------------------------------------------------------
// k_nn_lists_d<D> (nDims <= 32): the same lists from registers.  The kernel above reads both operands of every (x - y)^2 from LDS
// and fills 32 x 8 threads with the babies of a chain in groups of 32 (num_repeats = 40: 62 % of the slots); with several runs of a
// device in step it is the heaviest kernel of a round (1.6 ms for sixteen runs at BASELINE configs[3]).  Here a thread holds TWO
// babies' coordinates in registers (the loop over d is unrolled: one instantiation per nDims), the pairs of a chain share the
// workgroup with as many scanners each as fit (num_repeats 40: 20 pairs x 12 scanners = 240 threads), a staged point is read
// from LDS once for two babies, and a thread walks two points at a time (four sums side by side).  The same sums in the same order (d ascending, fused multiply-add of the
// difference), the same lists: ties between different points -- exact duplicates only -- go to the lower scanner, then the
// lower point, as above.
// ------------------------------------------------------------------------------------------
// the candidates of a nursery, once: every workgroup of k_nn_lists_d stages its tiles from this array with plain consecutive loads
// (resolving slot -> occupant -> row per workgroup was a chain of three dependent global loads per staged point: at nDims = 10 a
// workgroup spent four fifths of its time there)
// (use_rank: k_sort_live has just ranked the live set -- the snapshot's points go to the place of their rank, death order, and the empty
//  slots nowhere; k_nn_lists_d then finds the points that cannot die before a chain is looked at as ONE range.  Else: slot order.)
__device__ __forceinline__ void nn_gather_body(const PcState &S, int nleft, int use_rank)
{
    const int D = S.D, nr = S.nr, nT = S.nT, Ncap = S.Ncap;
    const int e = blockIdx.x * 256 + threadIdx.x, n = (Ncap + nleft) * D;
    if (e >= n) return;
    const int gi = e / D, d = e - gi * D;
    int code = PC_NN_NONE, pos = gi; double v = 0.0;
    if (gi < Ncap) {
        if (S.live_cluster[gi] >= 0) {
            code = gi; const int src = S.slot_src[gi]; v = (src >= 0) ? S.babies[((size_t)src * nr + (nr - 1)) * nT + d] : S.live[(size_t)gi * nT + d];
            if (use_rank) pos = S.nn_code[(size_t)Ncap + S.B + gi];
        } else if (use_rank) return;
        if (pos < 0 || pos >= Ncap) return;           // (a slot the sort did not see: not a candidate of this nursery)
    } else { const int c = gi - Ncap; code = -(1 + c); v = S.babies[((size_t)c * nr + (nr - 1)) * nT + d]; }
    S.nn_pts[(size_t)pos * D + d] = v;
    if (d == 0) S.nn_code[pos] = code;
}
__global__ __launch_bounds__(256) void k_nn_gather(PcState S, int nleft, int use_rank) { nn_gather_body(S, nleft, use_rank); }
__global__ __launch_bounds__(256) void k_nn_gather_many(const PcManyRec *__restrict__ R, int use_rank) { const PcManyView r = pc_many_view(R, blockIdx.y); nn_gather_body(r.S, r.ia[PC_REC_I_NLEFT], use_rank); }

#define NND_SC 16                                   /* at most this many scanners per pair of babies */
// Round 4: most of the candidates cannot die before the chain is looked at.  The deaths of a nursery take the snapshot's points in
// ascending logL (k_sort_live's order); before chain w is consumed at most ncand = nleft - 1 - w chains were, so a snapshot point of
// rank >= ncand is CERTAINLY alive then ("safe").  The nearest safe point ends every walk of a list: what the contraction needs is the
// candidates that may be dead by then ("uncertain": the ncand lowest snapshot points, the last babies of the chains before) that are
// NEARER than the nearest safe point, ascending, and then that point -- the old list of the eight nearest, cut off behind its first safe
// entry.  So a safe point costs a comparison (running minimum), and an uncertain one is inserted only if it beats that minimum: the
// sorted insertion, three quarters of the kernel's instructions while every candidate went through it, is now rare.  use_rank = 0 (no
// sorted order at hand): every candidate is uncertain, the old lists.
template <int D>
__device__ __forceinline__ void nn_lists_d_body(const PcState &S, int nleft, int tile_pts, int use_rank)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int DP = D | 1;                         // odd row stride: the scanners of a wave read different banks
    const int tid = threadIdx.x, nr = S.nr, nT = S.nT, Ncap = S.Ncap;
    const int w = blockIdx.x;                         // chain, w < nleft = entries still in the nursery
    double *pts = (double *)smem;                     // [tile_pts][DP]
    int *pcode = (int *)(pts + (size_t)tile_pts * DP);   // [tile_pts] code of each staged point, PC_NN_NONE = skip
    double *md = (double *)smem;                      // [256][2][PC_NN_K] merge buffer: over the tile, once the last one has been scanned
    int *mc = (int *)(md + 256 * 2 * PC_NN_K);        // [256][2][PC_NN_K]
    double *msd = (double *)smem;                     // [256][2] the scanners' nearest safe points (between the two scans)
    int *msc = (int *)(msd + 256 * 2);                // [256][2]
    if (w == 0) {                                     // liveness bookkeeping starts now
        for (int s = tid; s < Ncap; s += 256) S.nn_slot_owner[s] = -1;
        for (int c = tid; c < S.B; c += 256) S.nn_chain_slot[c] = -1;
    }
#ifdef NND_DBG
    long long nd_t[5] = {0, 0, 0, 0, 0}; long long nd_c = clock64(); const long long nd_start = nd_c;
#define NND_MARK(i) { const long long t_ = clock64(); nd_t[i] += t_ - nd_c; nd_c = t_; }
#else
#define NND_MARK(i)
#endif
    const int nc = S.ctl->ncluster;
    double Lg0 = S.logLp[0];
    for (int c = 1; c < nc; ++c) Lg0 = fmin(Lg0, S.logLp[c]);
    const double *blog = S.baby_logL + (size_t)w * nr;
    const int ncand = nleft - 1 - w;                  // chains w+1 .. nleft-1 are consumed before w
    // The gathered array (k_nn_gather).  use_rank: the snapshot's points stand in their death order (k_sort_live), n of them: the first
    // min(ncand, n) may be dead by the time this chain is looked at, the others cannot.  Without a sorted order at hand: slot order, all
    // of them uncertain (empty slots carry PC_NN_NONE).  Behind them, at Ncap, the last babies of the nursery's chains.
    const int *nn_rank = S.nn_code + (size_t)Ncap + S.B;
    const int nsnap = use_rank ? nn_rank[Ncap] : Ncap;
    const int nunc = use_rank ? (ncand < nsnap ? ncand : nsnap) : Ncap;      // uncertain snapshot entries: [0, nunc)
    const int nsafe = nsnap - nunc;                                          // safe ones: [nunc, nsnap)
    const int npair = (nr + 1) / 2;
    const int PG = npair < 256 ? npair : 256;         // pairs per pass
    const int nscan = (256 / PG) < NND_SC ? (256 / PG) : NND_SC;
    const int pi = tid / nscan, p = tid - pi * nscan;
    for (int pg0 = 0; pg0 < npair; pg0 += PG) {
        const bool act = pi < PG && pg0 + pi < npair;
        const int ia = 2 * (pg0 + pi), ib = ia + 1;
        double xa[D], xb[D];
        {
            const double *ra = S.babies + ((size_t)w * nr + (act ? ia : 0)) * nT, *rb = S.babies + ((size_t)w * nr + ((act && ib < nr) ? ib : 0)) * nT;
#pragma unroll
            for (int d = 0; d < D; ++d) { xa[d] = ra[d]; xb[d] = rb[d]; }
        }
        const bool minea = act && blog[ia] > Lg0;                 // the contour only rises: others never need a cluster
        const bool mineb = act && ib < nr && blog[ib] > Lg0;
        double bda[PC_NN_K], bdb[PC_NN_K]; int bca[PC_NN_K], bcb[PC_NN_K];
#pragma unroll
        for (int k = 0; k < PC_NN_K; ++k) { bda[k] = PC_HUGE; bdb[k] = PC_HUGE; bca[k] = PC_NN_NONE; bcb[k] = PC_NN_NONE; }
        double sa = PC_HUGE, sb = PC_HUGE; int sca = PC_NN_NONE, scb = PC_NN_NONE;      // nearest safe point: this scanner's, then the pair's
        auto insert = [&](double (&bd)[PC_NN_K], int (&bc)[PC_NN_K], double d2, int code) __attribute__((always_inline)) {
            double cd = d2; int cc = code;                        // sorted insertion, registers only (the caller has compared with the last entry)
#pragma unroll
            for (int k = 0; k < PC_NN_K; ++k) {
                const bool sw = cd < bd[k];
                const double td = sw ? bd[k] : cd; const int tc = sw ? bc[k] : cc;
                bd[k] = sw ? cd : bd[k]; bc[k] = sw ? cc : bc[k];
                cd = td; cc = tc;
            }
        };
        // one scan over `count` candidates, entry v of it = entry first + v of the gathered array (v < split) or the baby of chain
        // w + 1 + (v - split).  SAFE: a running minimum a point; else a sorted insertion for the few that beat the pair's nearest safe point.
        auto scan = [&](auto safe_tag, int first, int split, int count) __attribute__((always_inline)) {
            constexpr bool SAFE = decltype(safe_tag)::value;
            // (no early way out for an empty slot: with the sums used only inside a branch the compiler moved each of them INTO it, one
            //  dependent chain behind the other -- three times the latency of the four side by side)
            auto take = [&](double a0, double b0, int c0) __attribute__((always_inline)) {
                const bool is = c0 != PC_NN_NONE;
                if constexpr (SAFE) {
                    const bool ua = is & (a0 < sa), ub = is & (b0 < sb);
                    sa = ua ? a0 : sa; sca = ua ? c0 : sca;
                    sb = ub ? b0 : sb; scb = ub ? c0 : scb;
                } else {
                    if (is & minea & (a0 < bda[PC_NN_K - 1]) & (a0 < sa)) insert(bda, bca, a0, c0);
                    if (is & mineb & (b0 < bdb[PC_NN_K - 1]) & (b0 < sb)) insert(bdb, bcb, b0, c0);
                }
            };
            for (int t0 = 0; t0 < count; t0 += tile_pts) {
                const int tn = min(tile_pts, count - t0);
                __syncthreads();
                NND_MARK(2)
                for (int q = tid; q < tn; q += 256) { const int v = t0 + q; pcode[q] = S.nn_code[v < split ? first + v : Ncap + w + 1 + (v - split)]; }
                for (int e = tid; e < tn * D; e += 256) {
                    const int q = e / D, d = e - q * D, v = t0 + q;
                    pts[(size_t)q * DP + d] = S.nn_pts[(size_t)(v < split ? first + v : Ncap + w + 1 + (v - split)) * D + d];
                }
                __syncthreads();
                NND_MARK(1)
                if (minea || mineb) {
                    int q = p;
                    for (; q + nscan < tn; q += 2 * nscan) {          // two points at a time: four sums in flight
                        const int c0 = pcode[q], c1 = pcode[q + nscan];
                        const double *y0 = pts + (size_t)q * DP, *y1 = pts + (size_t)(q + nscan) * DP;
                        double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
#pragma unroll
                        for (int d = 0; d < D; ++d) {
                            const double u0 = y0[d], u1 = y1[d];
                            const double ta0 = xa[d] - u0, tb0 = xb[d] - u0, ta1 = xa[d] - u1, tb1 = xb[d] - u1;
                            a0 = fma(ta0, ta0, a0); b0 = fma(tb0, tb0, b0); a1 = fma(ta1, ta1, a1); b1 = fma(tb1, tb1, b1);
                        }
                        asm volatile("" : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1));      // (the four sums are made HERE, side by side)
                        take(a0, b0, c0); take(a1, b1, c1);
                    }
                    if (q < tn) {
                        const int c0 = pcode[q];
                        const double *y0 = pts + (size_t)q * DP;
                        double a0 = 0.0, b0 = 0.0;
#pragma unroll
                        for (int d = 0; d < D; ++d) { const double u0 = y0[d]; const double ta0 = xa[d] - u0, tb0 = xb[d] - u0; a0 = fma(ta0, ta0, a0); b0 = fma(tb0, tb0, b0); }
                        take(a0, b0, c0);
                    }
                }
            }
        };
        // Round 6: the safe points FIRST.  The list a walk needs is the uncertain candidates nearer than the pair's nearest safe point, and
        // then that point; while safe and uncertain candidates came mixed, a scanner measured an uncertain one against the nearest safe
        // point IT had seen so far, and nearly every iteration some lane of the wave made a sorted insertion -- eight compare-and-swap
        // steps on two register arrays, four fifths of the scan's cycles at nDims = 10.  Now the snapshot stands in death order: the
        // safe ones are a range, scanned first with a running minimum; the scanners' minima meet; and of the uncertain candidates
        // only those nearer than the PAIR's nearest safe point are inserted -- a handful per baby.
        scan(std::true_type{}, nunc, nsafe, nsafe);
        // the pair's nearest safe point: the scanners' minima meet (equal distances -- exact duplicates only -- go to the lower scanner)
        __syncthreads();                              // (the buffers lie over the tile)
        NND_MARK(2)
        msd[tid * 2 + 0] = sa; msc[tid * 2 + 0] = sca; msd[tid * 2 + 1] = sb; msc[tid * 2 + 1] = scb;
        __syncthreads();
        double fs[2] = {PC_HUGE, PC_HUGE}; int fc[2] = {PC_NN_NONE, PC_NN_NONE};
        if (act) {
            const int t0p = tid - p;                  // the pair's first scanner
#pragma unroll
            for (int h = 0; h < 2; ++h)
                for (int q = 0; q < nscan; ++q) { const double v = msd[(t0p + q) * 2 + h]; if (v < fs[h]) { fs[h] = v; fc[h] = msc[(t0p + q) * 2 + h]; } }
        }
        sa = fs[0]; sb = fs[1];
        scan(std::false_type{}, 0, nunc, nunc + ncand);
        // merge the partial lists of a baby: each is sorted, nscan-way pick by the pair's first scanner, up to the nearest safe point
        __syncthreads();
        NND_MARK(2)
#pragma unroll
        for (int k = 0; k < PC_NN_K; ++k) {
            md[(tid * 2 + 0) * PC_NN_K + k] = bda[k]; mc[(tid * 2 + 0) * PC_NN_K + k] = bca[k];
            md[(tid * 2 + 1) * PC_NN_K + k] = bdb[k]; mc[(tid * 2 + 1) * PC_NN_K + k] = bcb[k];
        }
        __syncthreads();
        if (act && p == 0) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = ia + h;
                if (i >= nr) continue;
                const bool mine = h ? mineb : minea;
                int head[NND_SC];
#pragma unroll
                for (int q = 0; q < NND_SC; ++q) head[q] = 0;
                int out[PC_NN_K];
                bool closed = false;                              // the safe point has been written: nothing behind it matters
#pragma unroll
                for (int k = 0; k < PC_NN_K; ++k) {
                    double best = PC_HUGE; int bq = -1;
#pragma unroll
                    for (int q = 0; q < NND_SC; ++q) {
                        const double v = (q < nscan && head[q] < PC_NN_K) ? md[((tid + q) * 2 + h) * PC_NN_K + head[q]] : PC_HUGE;
                        if (v < best) { best = v; bq = q; }
                    }
                    int code = PC_NN_NONE;
                    if (!closed && best < fs[h]) {
#pragma unroll
                        for (int q = 0; q < NND_SC; ++q) if (q == bq) { code = mc[((tid + q) * 2 + h) * PC_NN_K + head[q]]; head[q]++; }
                    } else if (!closed) { code = fc[h]; closed = true; }
                    out[k] = mine ? code : PC_NN_NONE;
                }
                int4 *dst = (int4 *)(S.nn_list + ((size_t)w * nr + i) * PC_NN_K);
                dst[0] = make_int4(out[0], out[1], out[2], out[3]);
                dst[1] = make_int4(out[4], out[5], out[6], out[7]);
            }
        }
        __syncthreads();
        NND_MARK(3)
    }
#ifdef NND_DBG
    if (w == 0 && tid == 0) {      // (chain 0: the most candidates) set-up / staging / scanning / merges, and the whole kernel in nn_fallbacks
        for (int x = 0; x < 4; ++x) atomicAdd((unsigned long long *)&S.ctl->gen_cyc[x], (unsigned long long)nd_t[x]);
        atomicAdd((unsigned long long *)&S.ctl->nn_fallbacks, (unsigned long long)(clock64() - nd_start));
    }
#endif
}
template <int D> __global__ __launch_bounds__(256) void k_nn_lists_d(PcState S, int nleft, int tile_pts, int use_rank) { nn_lists_d_body<D>(S, nleft, tile_pts, use_rank); }
template <int D> __global__ __launch_bounds__(256) void k_nn_lists_d_many(const PcManyRec *__restrict__ R, int tile_pts, int use_rank)
{
    const PcManyView r = pc_many_view(R, blockIdx.y);
    if ((int)blockIdx.x >= r.ia[PC_REC_I_NLEFT]) return;
    nn_lists_d_body<D>(r.S, r.ia[PC_REC_I_NLEFT], tile_pts, use_rank);
}
static size_t nn_lists_d_lds(const PcState *S, int &tile)
{
    const int DP = S->D | 1;
    const size_t merge = (sizeof(double) + sizeof(int)) * 256 * 2 * PC_NN_K;      // 48 KB, over the tile: three workgroups to a compute unit
    tile = (int)((merge - 64) / (sizeof(double) * DP + sizeof(int)));
    tile = tile < 32 ? 32 : (tile > 1024 ? 1024 : tile);
    tile &= ~1;                                       // (the codes lie behind tile x DP doubles: eight-byte aligned either way)
    const size_t t = (sizeof(double) * DP + sizeof(int)) * (size_t)tile;
    return (t > merge ? t : merge) + 64;
}
// nDims <= 32: the register kernel; dR == null: one run
static int nn_lists_d_dispatch(const PcState *S, const PcManyRec *dR, int R, int nleft, int use_rank, hipStream_t st)
{
    static const bool off = std::getenv("PC_NN_LISTS_OLD") != nullptr;
    if (off || S->D > 32 || S->D < 1) return 1;
    int tile;
    const size_t sh = nn_lists_d_lds(S, tile);
    if (!S->nn_pts) return 1;
    if (dR) hipLaunchKernelGGL(k_nn_gather_many, dim3(((S->Ncap + nleft) * S->D + 255) / 256, R), dim3(256), 0, st, dR, use_rank);
    else hipLaunchKernelGGL(k_nn_gather, dim3(((S->Ncap + nleft) * S->D + 255) / 256), dim3(256), 0, st, *S, nleft, use_rank);
    switch (S->D) {
#define PC_NND(n) case n: \
        if (dR) { pc_need_dyn_lds((const void *)k_nn_lists_d_many<n>, sh); \
                  hipLaunchKernelGGL(k_nn_lists_d_many<n>, dim3(nleft, R), dim3(256), sh, st, dR, tile, use_rank); } \
        else { pc_need_dyn_lds((const void *)k_nn_lists_d<n>, sh); \
               hipLaunchKernelGGL(k_nn_lists_d<n>, dim3(nleft), dim3(256), sh, st, *S, nleft, tile, use_rank); } \
        return 0;
        PC_NND(1) PC_NND(2) PC_NND(3) PC_NND(4) PC_NND(5) PC_NND(6) PC_NND(7) PC_NND(8) PC_NND(9) PC_NND(10) PC_NND(11) PC_NND(12) PC_NND(13) PC_NND(14) PC_NND(15) PC_NND(16)
        PC_NND(17) PC_NND(18) PC_NND(19) PC_NND(20) PC_NND(21) PC_NND(22) PC_NND(23) PC_NND(24) PC_NND(25) PC_NND(26) PC_NND(27) PC_NND(28) PC_NND(29) PC_NND(30) PC_NND(31) PC_NND(32)
#undef PC_NND
    }
    return 1;
}

static size_t nn_lists_lds(const PcState *S, int &tile)
{
    tile = (int)(24576 / (sizeof(double) * S->D));            // ~24 KB of coordinates per tile
    tile = tile < 16 ? 16 : (tile > 512 ? 512 : tile);
    return sizeof(double) * ((size_t)NNL_G * S->D + (size_t)tile * S->D + 256 * PC_NN_K) + sizeof(int) * (256 * PC_NN_K + tile) + 64;
}
// use_rank: k_sort_live has run on this state in front of this launch (its order tells which candidates cannot die before a chain is looked at)
extern "C" void pc_launch_nn_lists(const PcState *S, int nleft, int use_rank, hipStream_t st)
{
    if (nleft <= 0) return;
    if (nn_lists_d_dispatch(S, nullptr, 0, nleft, use_rank, st) == 0) return;
    int tile;
    const size_t sh = nn_lists_lds(S, tile);
    pc_need_dyn_lds((const void *)k_nn_lists, sh);
    hipLaunchKernelGGL(k_nn_lists, dim3(nleft), dim3(256), sh, st, *S, nleft, tile);
}
extern "C" int pc_launch_nn_lists_many(const PcState *S, const PcManyRec *dR, int R, int nleft_max, int use_rank, hipStream_t st)
{
    if (nleft_max <= 0) return 0;
    if (nn_lists_d_dispatch(S, dR, R, nleft_max, use_rank, st) == 0) return 0;
    int tile;
    const size_t sh = nn_lists_lds(S, tile);
    pc_need_dyn_lds((const void *)k_nn_lists_many, sh);
    hipLaunchKernelGGL(k_nn_lists_many, dim3(nleft_max, R), dim3(256), sh, st, dR, tile);
    return 0;
}

// dynamic nlive target (run_time_info.f90:766-771)
__device__ __forceinline__ int nlive_target(const PcState &S, double logL)
{
    int best = -1;
    for (int i = 0; i < S.n_nlives; ++i)
        if (logL > S.dyn_loglikes[i] && (best < 0 || S.dyn_loglikes[i] > S.dyn_loglikes[best])) best = i;
    return best < 0 ? S.N : S.dyn_nlives[best];
}

template <int NT>
// slots_global: the per-slot arrays (logL, cluster, list position, list owner) stay in HBM instead of LDS -- the way out
// for live sets beyond ~8000 points (20 B of LDS per slot); slower, same code
__global__ __launch_bounds__(NT) void k_consume(PcState S, int final_mode, int cache_x, int xq_n, int slots_global)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int Ncap = S.Ncap, maxc = S.maxc, nr = S.nr, nT = S.nT;
    ConsumeShared H;
    {
        char *p = smem;
        const bool sg0 = slots_global != 0;
        H.sL = sg0 ? S.live_logL : (double *)p; if (!sg0) p += sizeof(double) * Ncap;
        double **cd[] = { &H.cLogLp, &H.cLogXp, &H.cLogZp, &H.cLogZXp, &H.cLogZp2, &H.cLogZpXp, &H.cLseRef, &H.cLseSum, &H.cThr };
        for (int i = 0; i < 9; ++i) { *cd[i] = (double *)p; p += sizeof(double) * maxc; }
        H.jobres = (double *)p; p += sizeof(double) * NT;
        H.xbuf = (double *)p; p += sizeof(double) * S.D * PC_IDG;
        H.gd2 = (double *)p; p += sizeof(double) * NT;
        H.sX = (double *)p; H.xrows = cache_x; p += sizeof(double) * (size_t)cache_x * S.D;
        H.red = (vk_t *)p; p += sizeof(vk_t) * 16;
        H.sC = sg0 ? S.live_cluster : (int *)p; if (!sg0) p += sizeof(int) * Ncap;
        H.sP = sg0 ? S.live_pos : (int *)p; if (!sg0) p += sizeof(int) * Ncap;
        H.cN = (int *)p; p += sizeof(int) * maxc;
        H.cMinSlot = (int *)p; p += sizeof(int) * maxc;
        H.cUid = (unsigned *)p; p += sizeof(unsigned) * maxc;
        H.misc = (int *)p; p += sizeof(int) * 8;
        H.gkey = (int *)p; p += sizeof(int) * NT;
        H.ids = (int *)p; p += sizeof(int) * nr;
        H.sO = sg0 ? S.nn_slot_owner : (int *)p; if (!sg0) p += sizeof(int) * Ncap;
        H.sCS = (int *)p; p += sizeof(int) * S.B;
        p = (char *)(((size_t)p + 15) & ~(size_t)15);
        H.xq = (double *)p; H.xq_ld = xq_n;
    }
    PcCtl *ctl = S.ctl;
    // ---- stage the state in LDS
    const bool sg = slots_global != 0;
    if (!sg) for (int s = tid; s < Ncap; s += NT) { H.sL[s] = S.live_logL[s]; H.sC[s] = S.live_cluster[s]; H.sP[s] = S.live_pos[s]; }
    if (H.xrows >= Ncap) for (int e = tid; e < Ncap * S.D; e += NT) H.sX[e] = S.live[(size_t)(e / S.D) * nT + e % S.D];
    const bool nn = S.nn_valid != 0 && !final_mode;
    if (nn) {
        if (!sg) for (int s = tid; s < Ncap; s += NT) H.sO[s] = S.nn_slot_owner[s];
        for (int c = tid; c < S.B; c += NT) H.sCS[c] = S.nn_chain_slot[c];
    }
    int nc = ctl->ncluster;
    // the cross-volume matrix: every death reads and rewrites a row and a column of it; in global memory that is a
    // store -> load round trip per death (and 2 nc^2 of them, serially, when a cluster is deleted)
    const bool xq_lds = nc <= xq_n;                    // clusters only appear between launches
    if (xq_lds) { for (int e = tid; e < nc * nc; e += NT) H.xq[(size_t)(e / nc) * xq_n + e % nc] = S.XpXq[(size_t)(e / nc) * maxc + e % nc]; }
    else { H.xq = S.XpXq; H.xq_ld = maxc; }
    const int nc_at_launch = nc;
    for (int c = tid; c < maxc; c += NT) {
        H.cLogLp[c] = S.logLp[c]; H.cLogXp[c] = S.logXp[c]; H.cLogZp[c] = S.logZp[c]; H.cLogZXp[c] = S.logZXp[c];
        H.cLogZp2[c] = S.logZp2[c]; H.cLogZpXp[c] = S.logZpXp[c]; H.cLseRef[c] = S.lse_ref[c]; H.cLseSum[c] = S.lse_sum[c];
        H.cThr[c] = S.death_thr[c]; H.cN[c] = S.cl_n[c]; H.cMinSlot[c] = S.imin_slot[c]; H.cUid[c] = S.cl_uid[c];
    }
    // replicated scalars (every thread runs the same scalar code on the same inputs)
    int i_nursery = ctl->i_nursery, epoch = ctl->admin_epoch, failures = ctl->failures, ndead = ctl->ndead,
        nph = ctl->nphantom, nc_dead = ctl->ncluster_dead;
    long long nlike = ctl->nlike, niter = ctl->niter, nlike_failed = ctl->nlike_failed;
    double logZ = ctl->logZ, logZ2 = ctl->logZ2, lx_last = ctl->logX_last_update;
    unsigned next_uid = ctl->next_cluster_uid;
    int status = PC_ST_RUNNING, error = PC_ERR_NONE, cluster_deleted = 0;
    const int seg_hi = i_nursery - 1;
    double live_logZ_val = S.logzero, ll_m = -PC_HUGE, ll_s = 0.0;   // termination estimate, as value and as (max, sum) pair
    const double log2v = log(2.0);
    __syncthreads();
    // Reductions over the clusters, one cluster per lane.  Every wave computes them for itself from LDS: no barrier,
    // no broadcast (a serial loop over ~40 clusters with an exp each cost more than the rest of an iteration).
    // log sum_p X_p as a pair (m, s): the value is m + log s.  A fp64 log costs ~2000 cycles of latency on this serial
    // path; the update trigger compares in linear space and the posterior-stack column gets its log on the apply side.
    auto lse_logXp = [&](double &m_out, double &s_out) {
        if (nc == 1) { m_out = H.cLogXp[0]; s_out = 1.0; return; }
        double m = -PC_HUGE;
        for (int c0 = 0; c0 < nc; c0 += 64) { const int c = c0 + lane; m = fmax(m, c < nc ? H.cLogXp[c] : -PC_HUGE); }
        m = wave_max(m);
        double sum = 0.0;
        for (int c0 = 0; c0 < nc; c0 += 64) { const int c = c0 + lane; sum += (c < nc) ? exp(H.cLogXp[c] - m) : 0.0; }
        m_out = m; s_out = wave_sum<4>(sum);
    };
    auto lowest_contour = [&]() -> vk_t {              // (min_p logL_p, first cluster that has it): minpos
        if (nc == 1) return vk_t{H.cLogLp[0], 0};
        vk_t b{PC_HUGE, 0x7fffffff};
        for (int c0 = 0; c0 < nc; c0 += 64) { const int c = c0 + lane; if (c < nc) b = vk_min(b, vk_t{H.cLogLp[c], c}); }
        return wave_argmin(b);
    };

    // ================================================================================
    // one death: delete_outermost_point (run_time_info.f90:789-817) without the row copy
    // ================================================================================
    int last_cd = -1, last_pos_del = -1;
    double lx_m = 0.0, lx_s = 1.0; bool lx_known = false;   // log sum_p X_p = lx_m + log lx_s: only a death changes it
    int n_total = 0;                                   // live points over all clusters
    for (int c = 0; c < nc; ++c) n_total += H.cN[c];
    // Several waves, live set of a few thousand points: the three expensive parts of a death -- the evidence jobs (an exp and a
    // log each), the scan of the slots for the cluster's next minimum, the log-sum-exp of the volumes -- read only the state
    // before the death and do not need each other: the last wave takes the scan and the volumes while the others do the jobs,
    // and the state is rewritten once, behind one barrier (two barriers per death instead of seven; measured before: jobs
    // 2.5 k cycles, scan 2.3 k, volumes 0.8 k, one after the other).
    const bool fastkill = NT >= 256 && Ncap <= 4096 && !slots_global;
    const int ndead_kill0 = ndead;                            // (the kill-off's first death: its rows are copied behind the loop)
    auto kill_lowest = [&](int plan_w) {
        // cluster with the lowest contour (minpos: first minimum)
        const int cd = lowest_contour().k;
        const int n = H.cN[cd];
        n_total--;
        const double L = H.cLogLp[cd];
        const int slot_del = H.cMinSlot[cd];
        const int pos_del = H.sP[slot_del];
        last_cd = cd; last_pos_del = pos_del;
        // ---- update_evidence (run_time_info.f90:211-296): every log-space accumulation reads only
        //      pre-update values, so they are independent jobs: one lane each.
        const double l0 = S.logn[n], l1 = S.logn[n + 1], l2 = S.logn[n + 2];
        const double Xp = H.cLogXp[cd], XX = H.xq[(size_t)cd * H.xq_ld + cd];
        const double logweight = Xp - l1;
        if (fastkill && nc <= NT - 64 - 8) {
            constexpr int NJ = NT - 64;                       // job lanes; the last wave scans
            int new_min_slot = -1; double new_min_L = PC_HUGE;
            if (tid >= NJ) {
                // ---- delete_point (array_utils.f90:433-458) + find_min_loglikelihoods (run_time_info.f90:883-909): the dying slot
                //      is skipped (its label is cleared below, with the rest of the state), the last list element takes its place
                vk_t best{PC_HUGE, 0x7fffffff};
                int myslot = -1;
                for (int s0 = lane; s0 < Ncap; s0 += 256) {             // four labels in flight: members are rare (n_p of Ncap slots)
                    int lab[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) lab[u] = (s0 + 64 * u < Ncap) ? H.sC[s0 + 64 * u] : -1;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int s = s0 + 64 * u;
                        if (lab[u] != cd || s == slot_del) continue;
                        int p = H.sP[s];
                        if (p == n - 1) { p = pos_del; H.sP[s] = p; }
                        const vk_t cand{H.sL[s], p};
                        const vk_t nb = vk_min(best, cand);
                        if (nb.k != best.k || nb.v != best.v) myslot = s;
                        best = nb;
                    }
                }
                const vk_t mine = best;
                best = wave_argmin(best);
                if (n - 1 > 0) { if (myslot >= 0 && mine.k == best.k && mine.v == best.v) { H.misc[0] = myslot; H.jobres[NT - 3] = best.v; } }
                else if (lane == 0) { H.misc[0] = -1; H.jobres[NT - 3] = PC_HUGE; }
            }
            // log sum_p X_p after the death (the dying cluster's new volume substituted): the scanning wave's job, or that of the
            // last job wave when its lanes have nothing else to do (100 clusters: the scan alone is the long pole)
            const bool lse_sep = 8 + nc <= NJ - 64;
            if (lse_sep ? (tid >= NJ - 64 && tid < NJ) : (tid >= NJ)) {
                double m = -PC_HUGE;
                for (int c0 = 0; c0 < nc; c0 += 64) { const int c = c0 + lane; m = fmax(m, c < nc ? (c == cd ? Xp + l0 - l1 : H.cLogXp[c]) : -PC_HUGE); }
                m = wave_max(m);
                double sum = 0.0;
                for (int c0 = 0; c0 < nc; c0 += 64) { const int c = c0 + lane; sum += (c < nc) ? exp((c == cd ? Xp + l0 - l1 : H.cLogXp[c]) - m) : 0.0; }
                sum = wave_sum<4>(sum);
                if (nc == 1) { m = Xp + l0 - l1; sum = 1.0; }
                if (lane == 0) { H.jobres[NT - 1] = m; H.jobres[NT - 2] = sum; }
            }
            if (tid < (lse_sep ? NJ - 64 : NJ)) {
                double a = 0.0, b = 0.0, c3 = 0.0; bool has = false, has3 = false;
                if (tid == 0) { a = logZ; b = Xp + L - l1; has = true; }
                else if (tid == 1) { a = H.cLogZp[cd]; b = Xp + L - l1; has = true; }
                else if (tid == 2) { a = logZ2; b = log2v + H.cLogZXp[cd] + L - l1; c3 = log2v + XX + 2 * L - l1 - l2; has = has3 = true; }
                else if (tid == 3) { a = H.cLogZXp[cd] + l0 - l1; b = XX + L + l0 - l1 - l2; has = true; }
                else if (tid == 4) { a = H.cLogZp2[cd]; b = log2v + H.cLogZpXp[cd] + L - l1; c3 = log2v + XX + 2 * L - l1 - l2; has = has3 = true; }
                else if (tid == 5) { a = H.cLogZpXp[cd] + l0 - l1; b = XX + L + l0 - l1 - l2; has = true; }
                else if (tid == 6) { a = exp(L - H.cLseRef[cd]); }                       // live logsumexp bookkeeping
                else if (tid >= 8 && tid - 8 < nc && tid - 8 != cd && tid < NJ) {
                    const int q = tid - 8;
                    a = H.cLogZXp[q]; b = H.xq[(size_t)cd * H.xq_ld + q] + L - l1; has = true;
                }
                double r = a;
                if (has3) { const double m3 = fmax(a, fmax(b, c3)); r = m3 + log(exp(a - m3) + exp(b - m3) + exp(c3 - m3)); }
                else if (has) r = pc_logaddexp(a, b);
                H.jobres[tid] = r;
            }
            __syncthreads();
            logZ = H.jobres[0]; logZ2 = H.jobres[2];
            const double lxm = H.jobres[NT - 1], lxs = H.jobres[NT - 2];
            new_min_slot = H.misc[0]; new_min_L = H.jobres[NT - 3];
            if (tid == 0) {
                H.cLogZp[cd] = H.jobres[1]; H.cLogZXp[cd] = H.jobres[3]; H.cLogZp2[cd] = H.jobres[4]; H.cLogZpXp[cd] = H.jobres[5];
                H.cLogXp[cd] = Xp + l0 - l1;
                H.cLseSum[cd] -= H.jobres[6];
                H.cThr[cd] = L;
                H.cN[cd] = n - 1;
                H.sC[slot_del] = -1;
                if (nn) H.sO[slot_del] = -2;
                H.cMinSlot[cd] = new_min_slot; H.cLogLp[cd] = new_min_L;
            }
            if (tid < nc && tid != cd) H.cLogZXp[tid] = H.jobres[8 + tid];
            for (int q = tid; q < nc; q += NT) {
                if (q == cd) H.xq[(size_t)cd * H.xq_ld + cd] = XX + l0 - l2;
                else {
                    const double v = H.xq[(size_t)cd * H.xq_ld + q] + l0 - l1;
                    H.xq[(size_t)cd * H.xq_ld + q] = v; H.xq[(size_t)q * H.xq_ld + cd] = v;
                }
            }
            __syncthreads();                                  // (jobres is rewritten by the next death only after this)
            lx_m = lxm; lx_s = lxs; lx_known = true;
            if (ndead >= S.Dcap) { error = PC_ERR_DEAD_CAP; status = PC_ST_ERROR; }
            if (status != PC_ST_ERROR) {
                if (plan_w >= 0) {
                    if (tid == 0) {
                        const int src = S.slot_src[slot_del];
                        S.plan[plan_w].dead_idx = ndead;
                        S.plan[plan_w].dead_src = (src >= 0) ? -(1 + src) : slot_del;
                        S.plan[plan_w].logw = logweight; S.plan[plan_w].postX = lxm; S.plan[plan_w].postXs = lxs; S.plan[plan_w].postZ = logZ;
                        S.plan[plan_w].dead_cuid = H.cUid[cd];
                    }
                } else if (final_mode == 1) {
                    // the kill-off: nothing is born any more, the rows stay what they are -- they leave together behind the loop (a copy
                    // here is a global load and a store per death on the loop's critical path: a third of its 4.5 us)
                    if (tid == 0) {
                        S.sort_slot[ndead - ndead_kill0] = slot_del;
                        S.dead_logw[ndead] = logweight; S.dead_postX[ndead] = lxm + log(lxs); S.dead_postZ[ndead] = logZ;
                        S.dead_cuid[ndead] = H.cUid[cd];
                    }
                } else {   // trimming: rows are current in live[], copy immediately
                    const double *row = S.live + (size_t)slot_del * nT;
                    double *dst = S.dead + (size_t)ndead * nT;
                    for (int e = tid; e < nT; e += NT) dst[e] = row[e];
                    if (tid == 0) {
                        S.dead_logw[ndead] = logweight; S.dead_postX[ndead] = lxm + log(lxs); S.dead_postZ[ndead] = logZ;
                        S.dead_cuid[ndead] = H.cUid[cd]; S.dead_entry[ndead] = S.live_entry[slot_del];
                    }
                }
            }
            ndead++;
            return slot_del;
        }
        {
            double a = 0.0, b = 0.0, c3 = 0.0; bool has = false, has3 = false;
            if (tid == 0) { a = logZ; b = Xp + L - l1; has = true; }
            else if (tid == 1) { a = H.cLogZp[cd]; b = Xp + L - l1; has = true; }
            else if (tid == 2) { a = logZ2; b = log2v + H.cLogZXp[cd] + L - l1; c3 = log2v + XX + 2 * L - l1 - l2; has = has3 = true; }
            else if (tid == 3) { a = H.cLogZXp[cd] + l0 - l1; b = XX + L + l0 - l1 - l2; has = true; }
            else if (tid == 4) { a = H.cLogZp2[cd]; b = log2v + H.cLogZpXp[cd] + L - l1; c3 = log2v + XX + 2 * L - l1 - l2; has = has3 = true; }
            else if (tid == 5) { a = H.cLogZpXp[cd] + l0 - l1; b = XX + L + l0 - l1 - l2; has = true; }
            else if (tid == 6) { a = exp(L - H.cLseRef[cd]); }                       // live logsumexp bookkeeping
            else if (tid >= 8 && tid - 8 < nc && tid - 8 != cd && tid - 8 < NT - 8) {
                const int q = tid - 8;
                a = H.cLogZXp[q]; b = H.xq[(size_t)cd * H.xq_ld + q] + L - l1; has = true;
            }
            double r = a;
            if (has3) {                                 // one log instead of two nested logaddexp's
                const double m3 = fmax(a, fmax(b, c3));
                r = m3 + log(exp(a - m3) + exp(b - m3) + exp(c3 - m3));
            } else if (has) r = pc_logaddexp(a, b);
            H.jobres[tid] = r;
        }
        __syncthreads();
        // clusters beyond the lane budget (nc > NT-8): serial tail, rare
        for (int q = NT - 8 + tid; q < nc; q += NT)
            if (q != cd) H.cLogZXp[q] = pc_logaddexp(H.cLogZXp[q], H.xq[(size_t)cd * H.xq_ld + q] + L - l1);
        logZ = H.jobres[0]; logZ2 = H.jobres[2];
        const double nZp = H.jobres[1], nZXp = H.jobres[3], nZp2 = H.jobres[4], nZpXp = H.jobres[5], edel = H.jobres[6];
        __syncthreads();
        if (tid == 0) {
            H.cLogZp[cd] = nZp; H.cLogZXp[cd] = nZXp; H.cLogZp2[cd] = nZp2; H.cLogZpXp[cd] = nZpXp;
            H.cLogXp[cd] = Xp + l0 - l1;
            H.cLseSum[cd] -= edel;
            H.cThr[cd] = L;
            H.cN[cd] = n - 1;
            H.sC[slot_del] = -1;
            if (nn) H.sO[slot_del] = -2;
        }
        for (int q = tid; q < nc; q += NT) {
            if (q == cd) { if (true) H.xq[(size_t)cd * H.xq_ld + cd] = XX + l0 - l2; }
            else {
                if (q < NT - 8) H.cLogZXp[q] = H.jobres[8 + q];
                const double v = H.xq[(size_t)cd * H.xq_ld + q] + l0 - l1;
                H.xq[(size_t)cd * H.xq_ld + q] = v; H.xq[(size_t)q * H.xq_ld + cd] = v;
            }
        }
        __syncthreads();
        // ---- delete_point (array_utils.f90:433-458): the last list element moves into the hole;
        //      find_min_loglikelihoods (run_time_info.f90:883-909) for the shrunk cluster, one pass.
        vk_t best{PC_HUGE, 0x7fffffff};
        int myslot = -1;                               // slot of this thread's own candidate
        for (int s = tid; s < Ncap; s += NT) {
            if (H.sC[s] != cd) continue;
            int p = H.sP[s];
            if (p == n - 1) { p = pos_del; H.sP[s] = p; }
            const vk_t cand{H.sL[s], p};
            const vk_t nb = vk_min(best, cand);
            if (nb.k != best.k || nb.v != best.v) myslot = s;
            best = nb;
        }
        const vk_t mine = best;
        best = block_argmin<NT>(best, H.red);
        // slot of the new minimum: the thread whose own candidate (logL, pos) is the winner knows it (positions are unique)
        if (n - 1 > 0) {
            if (myslot >= 0 && mine.k == best.k && mine.v == best.v) { H.cMinSlot[cd] = myslot; H.cLogLp[cd] = best.v; }
        } else if (tid == 0) { H.cMinSlot[cd] = -1; H.cLogLp[cd] = PC_HUGE; }
        __syncthreads();
        // posterior-stack columns (calculate.f90:53-79): volume after the update, logZ after the update
        double lxm, lxs;
        lse_logXp(lxm, lxs);
        lx_m = lxm; lx_s = lxs; lx_known = true;
        if (ndead >= S.Dcap) { error = PC_ERR_DEAD_CAP; status = PC_ST_ERROR; }
        if (status != PC_ST_ERROR) {
            if (plan_w >= 0) {
                if (tid == 0) {
                    const int src = S.slot_src[slot_del];
                    S.plan[plan_w].dead_idx = ndead;
                    S.plan[plan_w].dead_src = (src >= 0) ? -(1 + src) : slot_del;
                    S.plan[plan_w].logw = logweight; S.plan[plan_w].postX = lxm; S.plan[plan_w].postXs = lxs; S.plan[plan_w].postZ = logZ;
                    S.plan[plan_w].dead_cuid = H.cUid[cd];
                }
            } else if (final_mode == 1) {      // (the kill-off: the rows leave together behind the loop, see above)
                if (tid == 0) {
                    S.sort_slot[ndead - ndead_kill0] = slot_del;
                    S.dead_logw[ndead] = logweight; S.dead_postX[ndead] = lxm + log(lxs); S.dead_postZ[ndead] = logZ;
                    S.dead_cuid[ndead] = H.cUid[cd];
                }
            } else {   // trimming: rows are current in live[], copy immediately
                const double *row = S.live + (size_t)slot_del * nT;
                double *dst = S.dead + (size_t)ndead * nT;
                for (int e = tid; e < nT; e += NT) dst[e] = row[e];
                if (tid == 0) {
                    S.dead_logw[ndead] = logweight; S.dead_postX[ndead] = lxm + log(lxs); S.dead_postZ[ndead] = logZ;
                    S.dead_cuid[ndead] = H.cUid[cd]; S.dead_entry[ndead] = S.live_entry[slot_del];
                }
            }
        }
        ndead++;
        return slot_del;
    };

    // delete_cluster (run_time_info.f90:507-598): drop the first empty cluster, keep the others' order
    int dropped_p = -1;
    auto drop_empty_cluster = [&]() -> bool {
        int p = -1;                                    // first empty cluster: one cluster per lane, every wave for itself
        for (int c0 = 0; c0 < nc && p < 0; c0 += 64) {
            const unsigned long long m = __ballot(c0 + lane < nc && H.cN[c0 + lane] == 0);
            if (m) p = c0 + __ffsll((long long)m) - 1;
        }
        if (p < 0) return false;
        __syncthreads();
        if (tid == 0) {
            if (nc_dead < S.maxc_dead) {
                S.logZp_dead[nc_dead] = H.cLogZp[p]; S.logZp2_dead[nc_dead] = H.cLogZp2[p]; S.cl_uid_dead[nc_dead] = H.cUid[p];
            }
        }
        nc_dead++;
        // XpXq compaction (row-major in place is safe: targets are lexicographically <= sources)
        if (tid == 0) {
            for (int a = 0, na = 0; a < nc; ++a) {
                if (a == p) continue;
                for (int b = 0, nb = 0; b < nc; ++b) { if (b == p) continue; H.xq[(size_t)na * H.xq_ld + nb] = H.xq[(size_t)a * H.xq_ld + b]; nb++; }
                na++;
            }
            for (int c = p; c < nc - 1; ++c) {
                H.cLogLp[c] = H.cLogLp[c + 1]; H.cLogXp[c] = H.cLogXp[c + 1]; H.cLogZp[c] = H.cLogZp[c + 1];
                H.cLogZXp[c] = H.cLogZXp[c + 1]; H.cLogZp2[c] = H.cLogZp2[c + 1]; H.cLogZpXp[c] = H.cLogZpXp[c + 1];
                H.cLseRef[c] = H.cLseRef[c + 1]; H.cLseSum[c] = H.cLseSum[c + 1]; H.cThr[c] = H.cThr[c + 1];
                H.cN[c] = H.cN[c + 1]; H.cMinSlot[c] = H.cMinSlot[c + 1]; H.cUid[c] = H.cUid[c + 1];
            }
        }
        const int DD = S.D * S.D;
        for (int c = p; c < nc - 1; ++c) {
            for (int e = tid; e < DD; e += NT) {
                S.chol[(size_t)c * DD + e] = S.chol[(size_t)(c + 1) * DD + e];
                S.cov[(size_t)c * DD + e] = S.cov[(size_t)(c + 1) * DD + e];
            }
            __syncthreads();
        }
        for (int s = tid; s < Ncap; s += NT) if (H.sC[s] > p) H.sC[s] -= 1;
        nc--;
        cluster_deleted = 1;
        dropped_p = p;
        __syncthreads();
        return true;
    };

    if (final_mode == 1) {
        // nested_sampling.F90:381-384: kill every remaining live point, lowest first
        while (nc > 0 && status == PC_ST_RUNNING) {
            kill_lowest(-1);
            drop_empty_cluster();
        }
        {   // the rows of the points that died here (the k-th death of the loop took slot sort_slot[k]): all threads, eight loads in flight
            __threadfence_block();
            __syncthreads();
            const int nk = ndead - ndead_kill0;
            const long long ne = (long long)nk * nT;
            for (long long e0 = tid; e0 < ne; e0 += (long long)NT * 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const long long e = e0 + (long long)u * NT;
                    if (e < ne) { const int k = (int)(e / nT), d = (int)(e - (long long)k * nT); v[u] = S.live[(size_t)((volatile int *)S.sort_slot)[k] * nT + d]; }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) { const long long e = e0 + (long long)u * NT; if (e < ne) S.dead[(size_t)ndead_kill0 * nT + e] = v[u]; }
            }
            for (int k = tid; k < nk; k += NT) S.dead_entry[ndead_kill0 + k] = S.live_entry[((volatile int *)S.sort_slot)[k]];
        }
        status = PC_ST_DONE;
    } else if (final_mode == 2) {
        // nested_sampling.F90:201-205: nprior > nlive, trim the initial set down to nlive
        while (H.cN[0] > S.N && status == PC_ST_RUNNING) kill_lowest(-1);
    }

    // ================================================================================
    // main loop: nested_sampling.F90:239-374 for the entries left in the nursery
    // ================================================================================
    long long cyT = 0, cyI = 0, cyK = 0, cyE = 0, cyF = 0, cyW = 0;
    bool live_changed = true;
    if (!final_mode && nc > 1) {
        // The nursery's records were written by other XCDs: a first touch costs 1-2 us, and the loop below would pay
        // that once per chain and array, serially.  Touch everything it will read now, in bulk, so that the loop's
        // loads hit this XCD's L2 (a few hundred KB at most).
        auto touch = [&](const void *base, size_t bytes) {
            const char *b = (const char *)base;
            for (size_t o = (size_t)tid * 64; o < bytes; o += (size_t)NT * 64) { const int v = *(const volatile int *)(b + o); asm volatile("" :: "v"(v)); }
        };
        touch(S.baby_logL, sizeof(double) * (size_t)i_nursery * nr);
        touch(S.ch_nlike, sizeof(int) * (size_t)i_nursery); touch(S.ch_epoch, sizeof(int) * (size_t)i_nursery); touch(S.ch_cluster, sizeof(int) * (size_t)i_nursery);
        if (nn) touch(S.nn_list, sizeof(int) * (size_t)i_nursery * nr * PC_NN_K);
        touch(S.slot_src, sizeof(int) * (size_t)Ncap);
        if (!xq_lds) for (int c = 0; c < nc; ++c) touch(S.XpXq + (size_t)c * maxc, sizeof(double) * (size_t)nc);
        // cube coordinates of every chain's last baby (they enter the LDS copy of the live set when the chain is accepted)
        for (int w2 = tid; w2 < i_nursery; w2 += NT) {
            const char *b = (const char *)(S.babies + ((size_t)w2 * nr + (nr - 1)) * nT);
            for (size_t o = 0; o < sizeof(double) * (size_t)S.D; o += 64) { const int v = *(const volatile int *)(b + o); asm volatile("" :: "v"(v)); }
        }
    }
    // The records of a chain -- its counters, the logL of its babies, their candidate lists -- are in L2 at best: three
    // dependent round trips per chain on this serial path.  They do not change during the launch: the next chain's are
    // requested while this one is processed.
    int pf_nlike = 0, pf_epoch = 0, pf_ca = 0;
    double pf_blog = 0.0, pf_last = 0.0;
    int4 pf_a = make_int4(PC_NN_NONE, PC_NN_NONE, PC_NN_NONE, PC_NN_NONE), pf_b = pf_a;
    auto prefetch_chain = [&](int wn) {
        if (wn < 0) return;
        pf_nlike = S.ch_nlike[wn]; pf_epoch = S.ch_epoch[wn]; pf_ca = S.ch_cluster[wn];
        const double *bl = S.baby_logL + (size_t)wn * nr;
        pf_blog = tid < nr ? bl[tid] : 0.0; pf_last = bl[nr - 1];
        if (nn && tid < nr) { const int4 *L4 = (const int4 *)(S.nn_list + ((size_t)wn * nr + tid) * PC_NN_K); pf_a = L4[0]; pf_b = L4[1]; }
    };
    if (!final_mode) prefetch_chain(i_nursery - 1);
    while (!final_mode && status == PC_ST_RUNNING) {
        const long long q0 = clock64();
        // ---- more_samples_needed (nested_sampling.F90:514-543) + failures guard (:239)
        bool more = true;
        if (S.max_ndead == 0) more = false;
        else if (S.max_ndead > 0 && ndead >= S.max_ndead) more = false;
        else if (S.use_prec) {
            // live_logZ (run_time_info.f90:683-709); per-cluster logsumexp kept incrementally.
            // One cluster per lane, log-sum-exp over the wave; the other waves pick the result up from LDS.
            // (a chain that replaced nothing left live set and evidence as they were: the estimate stands)
            if (live_changed)
            {   // every wave for itself (the state it reads was published before the last barrier of the iteration).
                // live_logZ = log sum_p exp(lse_p - log n_p + logX_p) with lse_p = ref_p + log(sum_p): kept as a pair
                // (mxv, acc), acc = sum_p (sum_p / n_p) exp(ref_p + logX_p - mxv) -- no log on the critical path
                double mxv = -PC_HUGE;
                for (int c0 = 0; c0 < nc; c0 += 64) {
                    const int c = c0 + lane;
                    mxv = fmax(mxv, (c < nc && H.cN[c] > 0) ? H.cLseRef[c] + H.cLogXp[c] : -PC_HUGE);
                }
                mxv = wave_max(mxv);
                double acc = 0.0;
                for (int c0 = 0; c0 < nc; c0 += 64) {
                    const int c = c0 + lane;
                    if (c < nc && H.cN[c] > 0) acc += (H.cLseSum[c] / ((double)H.cN[c] + 0.0)) * exp(H.cLseRef[c] + H.cLogXp[c] - mxv);
                }
                acc = wave_sum<4>(acc);
                ll_m = mxv; ll_s = acc;
            }
            // more_samples_needed: live_logZ < log(precision) + logZ   <=>   acc < exp(log(precision) + logZ - mxv)
            if (!(ll_s > 0.0) || ll_s < exp(S.log_prec + logZ - ll_m)) more = false;
        }
        if (!more || failures > S.nfail) { status = PC_ST_DONE; break; }
        if (i_nursery == 0) break;                      // batch exhausted: host launches the next one

        const long long q1 = clock64(); cyT += q1 - q0;
        const int w = i_nursery - 1;
        i_nursery--;
        const int n_total_before = n_total;
        live_changed = false;
        const int w_nlike = pf_nlike, w_epoch = pf_epoch, ca = pf_ca;
        const double my_blog = pf_blog, Llast_pf = pf_last;
        const int4 my_a = pf_a, my_b = pf_b;
        prefetch_chain(i_nursery - 1);
        nlike += w_nlike;
        niter++;
        if (tid == 0) { S.plan[w].dead_idx = -1; S.plan[w].ph_base = nph; S.plan[w].ph_count = 0; S.plan[w].contour = S.logzero; for (int m = 0; m < PC_MASK_WORDS; ++m) S.plan[w].ph_mask[m] = 0ull; }
        __syncthreads();
        if (w_epoch != epoch) { nlike_failed += w_nlike; continue; }   // nested_sampling.F90:313 epoch guard

        // ---- replace_point (run_time_info.f90:716-787)
        const double Lg = lowest_contour().v;
        const double *blog = S.baby_logL + (size_t)w * nr;
        if (tid == 0) S.plan[w].contour = Lg;
        // phantoms: babies 1..nr-1 that beat the global contour and fall in the seed cluster's cell
        int nph_add = 0;
        if (nc == 1) {
            for (int base = 0; base < nr - 1; base += NT) {
                const int i = base + tid;
                const bool f = (i < nr - 1) && ((base == 0 ? my_blog : blog[i]) > Lg);
                const unsigned long long m = __ballot(f);
                if (lane == 0 && m) S.plan[w].ph_mask[(base >> 6) + (tid >> 6)] = m;
                if (NT == 64) nph_add += __popcll(m);
            }
            if (NT > 64) {   // count after the masks are visible
                __syncthreads();
                for (int m = 0; m < (nr + 62) / 64; ++m) nph_add += __popcll(S.plan[w].ph_mask[m]);
            }
        } else {
            if (nn) {
                // identify_cluster from the candidate lists: the first entry that is alive NOW is the nearest live
                // point (everything nearer in the superset is dead or not yet born); one baby per thread
                int unresolved = 0;
                for (int i = tid; i < nr; i += NT) {
                    int res = -1;
                    if ((i == tid ? my_blog : blog[i]) > Lg) {
                        res = -2;
                        const int4 *L4 = (const int4 *)(S.nn_list + ((size_t)w * nr + i) * PC_NN_K);
                        const int4 a = (i == tid) ? my_a : L4[0], b = (i == tid) ? my_b : L4[1];
                        const int codes[PC_NN_K] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
                        for (int k = 0; k < PC_NN_K; ++k) {
                            const int code = codes[k];
                            if (res != -2 || code == PC_NN_NONE) continue;
                            const int s = code >= 0 ? code : H.sCS[-(1 + code)];
                            const bool alive = code >= 0 ? (H.sO[s] == -1) : (s >= 0 && H.sO[s] == -(1 + code));
                            if (alive) res = H.sC[s];
                        }
                        if (res == -2) unresolved = 1;
                    }
                    H.ids[i] = res;
                }
                cyW++;
                if (__syncthreads_or(unresolved)) { cyF++; block_identify_all<NT>(S, H, w, blog, Lg, nc, true); }
            } else block_identify_all<NT>(S, H, w, blog, Lg, nc);
            if (NT > 64 && nr <= NT) {
                // the masks of the 16 waves meet in LDS (scratch of the search); a store to the plan followed by a
                // load of the same words would cost a global round trip per chain
                const bool f = (tid < nr - 1) && (my_blog > Lg) && (H.ids[tid] == ca);
                const unsigned long long m = __ballot(f);
                if (lane == 0) { H.gkey[2 * (tid >> 6)] = (int)(unsigned)m; H.gkey[2 * (tid >> 6) + 1] = (int)(unsigned)(m >> 32); }
                __syncthreads();
                for (int q = 0; q < (nr + 62) / 64; ++q) nph_add += __popc((unsigned)H.gkey[2 * q]) + __popc((unsigned)H.gkey[2 * q + 1]);
                if (tid < PC_MASK_WORDS && tid < (nr + 62) / 64) {
                    const unsigned long long mm = ((unsigned long long)(unsigned)H.gkey[2 * tid + 1] << 32) | (unsigned)H.gkey[2 * tid];
                    if (mm) S.plan[w].ph_mask[tid] = mm;
                }
                __syncthreads();                       // gkey is reused by the next search
            } else {
                for (int base = 0; base < nr - 1; base += NT) {
                    const int i = base + tid;
                    const bool f = (i < nr - 1) && (blog[i] > Lg) && (H.ids[i] == ca);
                    const unsigned long long m = __ballot(f);
                    if (lane == 0 && m) S.plan[w].ph_mask[(base >> 6) + (tid >> 6)] = m;
                    if (NT == 64) nph_add += __popcll(m);
                }
                if (NT > 64) {   // count after the masks are visible
                    __syncthreads();
                    for (int m = 0; m < (nr + 62) / 64; ++m) nph_add += __popcll(S.plan[w].ph_mask[m]);
                }
            }
        }
        const long long q2 = clock64(); cyI += q2 - q1;
        if (nph + nph_add > S.Pcap) { status = PC_ST_ERROR; error = PC_ERR_PHANTOM_CAP; break; }
        if (tid == 0) S.plan[w].ph_cuid = H.cUid[ca];
        nph += nph_add;

        const double Llast = Llast_pf;
        bool replaced = false;
        if (Llast > Lg) {
            const int id = (nc == 1) ? 0 : H.ids[nr - 1];
            if (id == ca) {
                const int nl = nlive_target(S, Lg);
                int tot = n_total;
                int free_slot = -1;
                if (tot >= (nl > 1 ? nl : 1)) { free_slot = kill_lowest(w); replaced = true; tot--; }
                if (status == PC_ST_ERROR) break;
                if (tot < nl) {
                    if (free_slot < 0) {               // growing live set: take any free slot
                        if (tid == 0) H.misc[1] = -1;
                        __syncthreads();
                        for (int s = tid; s < Ncap; s += NT) if (H.sC[s] < 0) atomicMax(&H.misc[1], s);
                        __syncthreads();
                        free_slot = H.misc[1];
                        if (free_slot < 0) { status = PC_ST_ERROR; error = PC_ERR_NOSLOT; break; }
                    }
                    // add_point + find_min_loglikelihoods for the receiving cluster
                    if (tid == 0) {
                        const int pos = H.cN[ca];
                        H.sL[free_slot] = Llast; H.sC[free_slot] = ca; H.sP[free_slot] = pos;
                        H.cN[ca] = pos + 1;
                        if (pos == 0 || Llast < H.cLogLp[ca]) { H.cLogLp[ca] = Llast; H.cMinSlot[ca] = free_slot; }
                        // live logsumexp of the cluster
                        if (pos == 0) { H.cLseRef[ca] = Llast; H.cLseSum[ca] = 1.0; }
                        else if (Llast > H.cLseRef[ca]) { H.cLseSum[ca] = H.cLseSum[ca] * exp(H.cLseRef[ca] - Llast) + 1.0; H.cLseRef[ca] = Llast; }
                        else H.cLseSum[ca] += exp(Llast - H.cLseRef[ca]);
                        S.slot_src[free_slot] = w;
                        if (nn) { H.sO[free_slot] = w; H.sCS[w] = free_slot; }
                    }
                    n_total++;
                    if (H.xrows >= Ncap) for (int d = tid; d < S.D; d += NT) H.sX[(size_t)free_slot * S.D + d] = S.babies[((size_t)w * nr + nr - 1) * nT + d];
                    __syncthreads();
                    // engine rule (oracle keyed mode): a point that replaces a death of its own cluster
                    // takes the dead point's list position instead of being appended
                    if (!S.seq_mode && replaced && last_cd == ca && last_pos_del < H.cN[ca] - 1) {
                        const int pos_new = H.cN[ca] - 1;
                        for (int s = tid; s < Ncap; s += NT)
                            if (s != free_slot && H.sC[s] == ca && H.sP[s] == last_pos_del) H.sP[s] = pos_new;
                        __syncthreads();
                        if (tid == 0) H.sP[free_slot] = last_pos_del;
                        __syncthreads();
                    }
                }
            }
        } else {
            // failed spawn: the last baby is recorded as dead with zero weight (run_time_info.f90:781-785)
            if (ndead >= S.Dcap) { status = PC_ST_ERROR; error = PC_ERR_DEAD_CAP; break; }
            if (tid == 0) {
                S.plan[w].dead_idx = ndead; S.plan[w].dead_src = -(1 + w);
                S.plan[w].logw = S.logzero; S.plan[w].postX = 0.0; S.plan[w].postXs = 1.0; S.plan[w].postZ = 0.0; S.plan[w].dead_cuid = 0xFFFFFFFFu;
            }
            ndead++;
        }
        failures = replaced ? 0 : failures + 1;
        if (!replaced) nlike_failed += w_nlike;
        live_changed = replaced || n_total != n_total_before;
        const long long q3 = clock64(); cyK += q3 - q2;

        // ---- update trigger (nested_sampling.F90:321) and delete_cluster (:339)
        if (!lx_known) { lse_logXp(lx_m, lx_s); lx_known = true; }
        // nested_sampling.F90:321  logsumexp(logXp) <= logX_last_update + log(compression_factor), in linear space
        const bool update = lx_s <= exp(lx_last + S.log_cf - lx_m);
        if (update) lx_last = lx_m + log(lx_s);
        if (drop_empty_cluster()) {
            if (S.epoch_discard) epoch++;          // nested_sampling.F90:339-341 as written: every chain in flight fails the guard of :313
            else {
                // the engine's rule (oracle: remap_chains): only the chains seeded in the cluster that ended are lost; the clusters behind
                // it moved up one place and the chains seeded in them follow
                const int p = dropped_p;
                for (int w2 = tid; w2 < i_nursery; w2 += NT) {
                    const int c = S.ch_cluster[w2];
                    if (c == p) { S.ch_cluster[w2] = -1; S.ch_epoch[w2] = -1; }
                    else if (c > p) S.ch_cluster[w2] = c - 1;
                }
                if (pf_ca == p) { pf_ca = -1; pf_epoch = -1; } else if (pf_ca > p) pf_ca -= 1;      // (the next chain's record is in registers already)
                __syncthreads();
            }
        }
        cyE += clock64() - q3;
        if (nc == 0) { status = PC_ST_DONE; break; }
        if (update) { status = PC_ST_UPDATE; break; }
    }

    // ---- write the state back
    __syncthreads();
    if (!sg) for (int s = tid; s < Ncap; s += NT) { S.live_logL[s] = H.sL[s]; S.live_cluster[s] = H.sC[s]; S.live_pos[s] = H.sP[s]; }
    for (int s = tid; s < Ncap; s += NT) if (H.sC[s] >= 0) S.cl_list[(size_t)H.sC[s] * Ncap + H.sP[s]] = s;
    if (xq_lds) {                                      // (a deleted cluster leaves stale entries beyond nc: never read)
        for (int e = tid; e < nc_at_launch * nc_at_launch; e += NT) S.XpXq[(size_t)(e / nc_at_launch) * maxc + e % nc_at_launch] = H.xq[(size_t)(e / nc_at_launch) * xq_n + e % nc_at_launch];
    }
    if (nn) {
        if (!sg) for (int s = tid; s < Ncap; s += NT) S.nn_slot_owner[s] = H.sO[s];
        for (int c = tid; c < S.B; c += NT) S.nn_chain_slot[c] = H.sCS[c];
    }
    for (int c = tid; c < maxc; c += NT) {
        S.logLp[c] = H.cLogLp[c]; S.logXp[c] = H.cLogXp[c]; S.logZp[c] = H.cLogZp[c]; S.logZXp[c] = H.cLogZXp[c];
        S.logZp2[c] = H.cLogZp2[c]; S.logZpXp[c] = H.cLogZpXp[c]; S.lse_ref[c] = H.cLseRef[c]; S.lse_sum[c] = H.cLseSum[c];
        S.death_thr[c] = H.cThr[c]; S.cl_n[c] = H.cN[c]; S.imin_slot[c] = H.cMinSlot[c]; S.cl_uid[c] = H.cUid[c];
    }
    if (tid == 0) {
        ctl->status = status; ctl->error = error; ctl->i_nursery = i_nursery; ctl->admin_epoch = epoch;
        ctl->failures = failures; ctl->ncluster = nc; ctl->ncluster_dead = nc_dead; ctl->ndead = ndead;
        ctl->nphantom = nph; ctl->seg_hi = seg_hi; ctl->seg_lo = i_nursery; ctl->cluster_deleted = cluster_deleted;
        ctl->next_cluster_uid = next_uid; ctl->nlike = nlike; ctl->niter = niter; ctl->nlike_failed = nlike_failed;
        if (ll_s > 0.0) { const double v = ll_m + log(ll_s); live_logZ_val = (v > S.logzero + 800.0) ? v : pc_logaddexp(S.logzero, v); }
        ctl->logZ = logZ; ctl->logZ2 = logZ2; ctl->logX_last_update = lx_last; ctl->live_logZ = live_logZ_val;
        ctl->gen_cyc[0] += cyT; ctl->gen_cyc[1] += cyI; ctl->gen_cyc[2] += cyK; ctl->gen_cyc[3] += cyE; ctl->nn_walks += cyW; ctl->nn_fallbacks += cyF;
    }
    pc_publish_ctl(S);
}

// ------------------------------------------------------------------------------------------
// initial values of the per-cluster state and of the control block (initialise_run_time_info,
// run_time_info.f90:164-206): one launch instead of a dozen small host copies
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_init_state(PcState S, double logzero)
{
    const int tid = threadIdx.x, maxc = S.maxc, D = S.D;
    for (int m = tid; m < maxc; m += 256) {
        S.logZp[m] = logzero; S.logZXp[m] = logzero; S.logZp2[m] = logzero; S.logZpXp[m] = logzero; S.logLp[m] = logzero;
        S.logXp[m] = 0.0; S.lse_ref[m] = 0.0; S.lse_sum[m] = 0.0; S.death_thr[m] = -PC_HUGE;
        S.cl_n[m] = 0; S.cl_uid[m] = 0u; S.imin_slot[m] = 0;
    }
    for (int e = tid; e < maxc * maxc; e += 256) S.XpXq[e] = 0.0;
    for (size_t e = tid; e < (size_t)maxc * D * D; e += 256) {
        const int r = (int)(e % ((size_t)D * D));
        const double v = (r / D == r % D) ? 1.0 : 0.0;
        S.chol[e] = v; S.cov[e] = v;
    }
    if (tid == 0) {
        PcCtl c0{};
        c0.status = PC_ST_RUNNING; c0.ncluster = 1; c0.logZ = logzero; c0.logZ2 = logzero;
        c0.logX_last_update = 0.0; c0.next_cluster_uid = 1; c0.live_logZ = logzero;
        *S.ctl = c0;
    }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
static size_t consume_lds(const PcState *S, int NT, int xrows, int xq_n = 0, int slots_global = 0)
{
    if (xq_n > 0) return consume_lds(S, NT, xrows, 0, slots_global) + sizeof(double) * (size_t)xq_n * xq_n + 16;
    const size_t nslot = slots_global ? 0 : (size_t)S->Ncap;
    return sizeof(double) * (nslot + 9 * (size_t)S->maxc + 2 * NT + (size_t)S->D * PC_IDG + (size_t)xrows * S->D) +
           sizeof(vk_t) * 16 + sizeof(int) * (3 * nslot + 3 * (size_t)S->maxc + 8 + NT + S->nr + (size_t)S->B) + 64;
}
// the per-slot arrays do not fit next to the smallest coordinate tile: keep them in HBM
static int consume_slots_global(const PcState *S, int NT) { return consume_lds(S, NT, 32) > 150 * 1024; }

extern "C" int pc_launch_consume(const PcState *S, int final_mode, int wide, hipStream_t st)
{
    // With the candidate lists the heavy parallel part (the nearest-cluster search) is gone and what is left is barriers
    // and short scans: 256 threads (4 waves) run it 1.4x faster than 1024 (16 waves, 128-VGPR cap).  PC_CONSUME_NT overrides.
    static const int wide_nt = std::getenv("PC_CONSUME_NT") ? std::atoi(std::getenv("PC_CONSUME_NT")) : 256;
    if (wide && (S->nn_valid || final_mode == 1) && wide_nt != 1024) {
#define PC_CONSUME_LAUNCH(NTV) { \
            /* the lists make the coordinate cache a fallback: a tile is enough, the LDS goes to the cross-volume matrix */ \
            const int sgl = consume_slots_global(S, NTV); \
            int cache_x = S->Ncap < 64 ? S->Ncap : 64, xq_n = S->maxc; \
            while (xq_n > 8 && consume_lds(S, NTV, cache_x, xq_n, sgl) > 158 * 1024) xq_n -= 8; \
            const size_t sh = consume_lds(S, NTV, cache_x, xq_n, sgl); \
            if (sh > 160 * 1024) return 1; \
            pc_need_dyn_lds((const void *)k_consume<NTV>, sh); \
            hipLaunchKernelGGL((k_consume<NTV>), dim3(1), dim3(NTV), sh, st, *S, final_mode, cache_x, xq_n, sgl); \
            return 0; }
        if (wide_nt == 64) PC_CONSUME_LAUNCH(64)
        if (wide_nt == 128) PC_CONSUME_LAUNCH(128)
        if (wide_nt == 512) PC_CONSUME_LAUNCH(512)
        PC_CONSUME_LAUNCH(256)
#undef PC_CONSUME_LAUNCH
    }
    if (wide) {
        // all live coordinates in LDS when they fit, else the largest tile that does
        const int sgl = consume_slots_global(S, 1024);
        int cache_x = S->Ncap;
        while (cache_x > 32 && consume_lds(S, 1024, cache_x, 0, sgl) > 158 * 1024) cache_x = (cache_x + 1) / 2;
        const size_t sh = consume_lds(S, 1024, cache_x, 0, sgl);
        if (sh > 160 * 1024) return 1;
        pc_need_dyn_lds((const void *)k_consume<1024>, sh);
        hipLaunchKernelGGL((k_consume<1024>), dim3(1), dim3(1024), sh, st, *S, final_mode, cache_x, 0, sgl);
    } else {
        const int sgl = consume_slots_global(S, 64);
        int xr = S->Ncap;
        while (xr > 32 && consume_lds(S, 64, xr, 0, sgl) > 158 * 1024) xr = (xr + 1) / 2;
        const size_t sh = consume_lds(S, 64, xr, 0, sgl);
        if (sh > 160 * 1024) return 1;
        pc_need_dyn_lds((const void *)k_consume<64>, sh);
        hipLaunchKernelGGL((k_consume<64>), dim3(1), dim3(64), sh, st, *S, final_mode, xr, 0, sgl);
    }
    return 0;
}

extern "C" void pc_launch_init_state(const PcState *S, double logzero, hipStream_t st)
{
    hipLaunchKernelGGL(k_init_state, dim3(1), dim3(256), 0, st, *S, logzero);
}
