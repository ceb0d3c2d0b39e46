// pc_sample.hip -- the kernels that evaluate the user's problem: the prior transform, the likelihood on a wave,
// prior sampling of the initial live set, the maximiser and the batched slice-sampling chains (K1).
// pc_rtc.hip compiles this very text a second time at run time (with pc_dev.h, pc_state.h, pc_seed.h and
// pc_slice_body.inc) for a device-source handle; every launcher below goes through PC_LAUNCH.
//
// One nursery batch = B independent chains, all seeded from one snapshot of the live set:
// exactly the reference's synchronous farm with nprocs-1 = B
// (src/polychord/nested_sampling.F90:262-286), but the "workers" are wavefronts.
//
//   K0           the chains' random whitened directions: pc_bases.hip, a translation unit of its own
//                (nothing there depends on the user's problem); the seed choice and the deck that both
//                sides need are pc_seed.h.
//   K1 k_slice   one wavefront per chain; lane d owns cube coordinate d (+64k).  Restates
//                SliceSampling / slice_sample (chordal_sampling.f90:7-92, 163-273) and
//                calculate_point (calculate.f90:6-50); likelihood sums are DPP butterflies.
#include "pc_state.h"
#include "pc_seed.h"
#ifndef __HIPCC_RTC__
#include <cstdlib>
#endif

// ------------------------------------------------------------------------------------------
// likelihood on a wave: lane owns DPL coordinates (dim = lane + 64*k)
// ------------------------------------------------------------------------------------------
template <int DPL>
struct LaneDims {
    double lo[DPL], span[DPL];   // uniform prior box (priors.f90:40-55)
    double mean[DPL];            // corr gaussian mean / twin gaussian means are derived
    bool on[DPL];
};

// ------------------------------------------------------------------------------------------
// prior table (PcPrior::kind == 2, the reference's prior types: priors.f90:40-290, hypercube_to_physical :494-556) on a wave, lane =
// PARAMETER.  S.prior.lo carries the doubles [3][D] -- per base type: uniform lo, hi - lo; log_uniform lo, hi / lo; power_uniform
// a = lo^(1/p), |a - hi^(1/p)|, p; gaussian / half_gaussian mu, sigma; exponential the rate -- S.prior.hi the integers [6][D] (base type
// 1 .. 6, 1-based position in the sorted_ block and the block's length or 0, 0, hypercube index, and for a member of an adaptive block --
// priors.f90:363-488 -- the hypercube index of its count's and of its layer's coordinate, else -1), S.src_pad the wave-uniform mask:
// bit t = base type t is present, bit 16 = a sorted_ or adaptive block, bit 17 = the hypercube order is no identity, bit 18 = an adaptive
// block, bit 19 = a layer parameter (nn_adaptive_layer_gaussian).  Read ONCE at the head of a chain.
// An adaptive block's count (and layer) parameter is a uniform entry here: lo 0.5, span = the number of members (2).  Its members carry
// pos = 1-based position among the members and len = their number; how many of them are order statistics is the POINT's (pc_table_theta).
// ------------------------------------------------------------------------------------------
// the uniform box at one coordinate, span = hi - lo: ONE expression for every kernel that forms it outside the chord (the live points, the
// maximiser, the blocks of the device batch callback), so that they agree to the bit -- the compiler contracts it to an fma, as it does the
// uniform entry of a table below
__device__ __forceinline__ double pc_box_theta(double lo, double span, double cube) { return lo + span * cube; }
#define PC_PT_SORTED (1u << 16)
#define PC_PT_PERMUTED (1u << 17)
#define PC_PT_ADAPTIVE (1u << 18)
#define PC_PT_LAYER (1u << 19)
template <int DPL>
struct LaneTable {
    int type[DPL], pos[DPL], len[DPL], hyp[DPL];
    int cnt[DPL], lay[DPL];      // a member of an adaptive block: hypercube index of its count's and of its layer's coordinate, else -1
    double p0[DPL], p1[DPL], p2[DPL];
    unsigned mask;
};
// AD (here and in pc_table_theta): the text knows adaptive blocks.  k_slice / k_slice_many carry it as PT = 2, a template value of its own, so
// that the PT = 1 kernels of every other table are instruction for instruction what they were (with the adaptive text inside, the sorted
// table's k_slice took 4 % longer a launch: profiles/adaptive_priors.json); the kernels off the hot path have the one text, AD = true.
template <int DPL, bool AD>
__device__ __forceinline__ void pc_table_load(const PcState &S, int lane, LaneTable<DPL> &lt)
{
    const int D = S.D;
    const double *tp = S.prior.lo;
    const int *ti = (const int *)S.prior.hi;
    lt.mask = (unsigned)S.src_pad;
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        const int dim = lane + 64 * k;
        const bool on = dim < D;
        lt.type[k] = on ? ti[dim] : 0; lt.pos[k] = on ? ti[D + dim] : 0; lt.len[k] = on ? ti[2 * D + dim] : 0; lt.hyp[k] = on ? ti[3 * D + dim] : 0;
        lt.p0[k] = on ? tp[dim] : 0.0; lt.p1[k] = on ? tp[D + dim] : 0.0; lt.p2[k] = on ? tp[2 * D + dim] : 0.0;
        if constexpr (AD) {
            lt.cnt[k] = -1; lt.lay[k] = -1;
            if (lt.mask & PC_PT_ADAPTIVE) {               // (wave-uniform: a run without such a block reads nothing more)
                lt.cnt[k] = on ? ti[4 * D + dim] : -1; lt.lay[k] = on ? ti[5 * D + dim] : -1;
            }
        }
    }
}
// nfunc of an adaptive block with n1 members at its count coordinate x (priors.f90:378-380): INT((0.5 + x n1) + 0.5), each operation
// rounded on its own as on the host (pc_adaptive_nfunc, pc_prior_table.h: no fma, or a point one ulp beside a bin edge sorts another number
// of members than the host does), clamped to 1 .. n1 as there
__device__ __forceinline__ int pc_table_nfunc(double x, int n1)
{
    const int nf = (int)__dadd_rn(__dadd_rn(0.5, __dmul_rn(x, (double)n1)), 0.5);
    return nf < 1 ? 1 : (nf > n1 ? n1 : nf);
}
// a member of an adaptive block at one point: nfn = the length of the sorted part it belongs to (0: it keeps y = x), and whether its
// layer coordinate asks for the half_gaussian base (theta_1 = 0.5 + 2 x < 1.5, priors.f90:480-486; 2 x is exact).  cube_h: the staged cube
template <int DPL>
__device__ __forceinline__ void pc_table_adapt(const LaneTable<DPL> &lt, const double *cube_h, int (&nfn)[DPL], bool (&half)[DPL])
{
#pragma unroll
    for (int k = 0; k < DPL; ++k)
        if (lt.cnt[k] >= 0) {
            const int nf = pc_table_nfunc(cube_h[lt.cnt[k]], lt.len[k]);
            nfn[k] = lt.pos[k] <= nf ? nf : 0;
            if (lt.mask & PC_PT_LAYER) { if (lt.lay[k] >= 0) half[k] = __dadd_rn(0.5, cube_h[lt.lay[k]] * 2.0) < 1.5; }
        }
}
// cube (hypercube order) -> theta (parameter order).  ybuf: the wave's LDS scratch of >= D doubles (one wave per workgroup: the barriers
// are cheap and every lane reaches them -- the mask is a kernel argument).  A wave pays each type PRESENT in the run once per call:
//   * y = cube[hyper[dim]]: a gather through LDS unless the order is the identity;
//   * adaptive blocks: every member reads its block's count coordinate (and its layer's) from the staged cube -- staged for the gather
//     already, else here -- and forms nfunc; the first nfunc members are a sorted_ block whose last member is count + nfunc, the others
//     keep y = x;
//   * sorted_ blocks (priors.f90:245-262): every member forms x_j^(1/j) (one pow a lane), then the running product from the block's LAST member down to
//     its own, in the reference's order of multiplication (y_n = x_n^(1/n), y_k = y_{k+1} x_k^(1/k)): a short serial chain a lane over
//     LDS, all members in parallel; a block may lie across the lane-63 / lane-0 boundary;
//   * the separable transform of the lane's type; the types that are absent from the run are skipped by a scalar branch.
template <int DPL, bool AD>
__device__ __forceinline__ void pc_table_theta(const LaneTable<DPL> &lt, const double (&cube)[DPL], double (&th)[DPL], int lane, double *ybuf)
{
    double y[DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) y[k] = cube[k];
    int nfn[DPL];               // length of the sorted part this lane's coordinate is a member of: the block's, or the point's nfunc
    bool half[DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) { nfn[k] = lt.len[k]; half[k] = false; }
    if (lt.mask & PC_PT_PERMUTED) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (lt.type[k]) ybuf[lane + 64 * k] = cube[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (lt.type[k]) y[k] = ybuf[lt.hyp[k]];
        if constexpr (AD) { if (lt.mask & PC_PT_ADAPTIVE) pc_table_adapt<DPL>(lt, ybuf, nfn, half); }
        __syncthreads();
    } else if (AD && (lt.mask & PC_PT_ADAPTIVE)) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (lt.type[k]) ybuf[lane + 64 * k] = cube[k];
        __syncthreads();
        pc_table_adapt<DPL>(lt, ybuf, nfn, half);
        __syncthreads();
    }
    if (lt.mask & PC_PT_SORTED) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            if (nfn[k] > 0) {
                const int j = lt.pos[k];
                double t = pow(y[k], 1.0 / (double)j);
                // (within 2^-33 of 1 the root is formed exactly, as on the host -- pc_sorted_root, pc_prior_table.h: the last bit of pow
                //  would decide there whether the block's largest member meets the p >= 1 guard of AS241)
                if (y[k] < 1.0 && y[k] > 1.0 - 0x1p-33 && j <= 256) {
                    const int kk = (int)((1.0 - y[k]) * 0x1p53);
                    t = 1.0 - (double)((2 * kk + j) / (2 * j)) * 0x1p-53;
                }
                y[k] = t;
            }
            if (lt.type[k]) ybuf[lane + 64 * k] = y[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DPL; ++k)
            if (nfn[k] > 0) {
                const int dim = lane + 64 * k, last = dim - lt.pos[k] + nfn[k];
                double r = ybuf[last];
                for (int i = last - 1; i >= dim; --i) r = r * ybuf[i];
                y[k] = r;
            }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        int t = lt.type[k];
        if constexpr (AD) { if (lt.mask & PC_PT_LAYER) { if (half[k]) t = 5; } }
        double v = 0.0;
        if (lt.mask & (1u << 1)) { if (t == 1) v = lt.p0[k] + lt.p1[k] * y[k]; }                          // priors.f90:40-55
        if (lt.mask & (1u << 2)) { if (t == 2) v = lt.p0[k] * pow(lt.p1[k], y[k]); }                      // :114-128
        if (lt.mask & (1u << 3)) { if (t == 3) v = pow(lt.p0[k] - y[k] * lt.p1[k], lt.p2[k]); }           // :151-167
        if (lt.mask & ((1u << 4) | (1u << 5))) {                                                          // :73-88, :172-187
            if (t == 4 || t == 5) v = lt.p0[k] + lt.p1[k] * pc_inv_normal_cdf(t == 4 ? y[k] : 0.5 + 0.5 * y[k]);
        }
        if (lt.mask & (1u << 6)) { if (t == 6) v = -log(1.0 - y[k]) / lt.p0[k]; }                         // :192-204
        th[k] = v;
    }
}

// The one entry point of the transform: every kernel that turns a cube into theta behind a prior table goes through PC_PRIOR_LOAD (the
// head of a chain) and PC_PRIOR_THETA (every trial).  Without a user prior they ARE pc_table_load and pc_table_theta, token for token.
#ifdef PCHIP_USER_PRIOR
// A user's prior written as device source (PcPrior::kind == 3, pchip_source_create_prior; pc_rtc.hip defines PCHIP_USER_PRIOR in front of
// this text in such a handle's unit): theta[i] = pchip_prior_param(cube, i, ...), one call per parameter, lane = parameter.  The function
// may read ANY coordinate of the cube (a dependent prior loops in its lane, as the sorted_ blocks above do), so the cube is staged in the
// wave's LDS scratch first: write / barrier / read / barrier, the shape of the table's permuted gather.  Only ever called for points
// inside the unit cube (calculate.f90:36-38 stays in front, where it is for a table).
__device__ double pchip_prior_param(const double *cube, int i, int nDims, const double *data, long ndata);

template <int DPL>
__device__ __forceinline__ void pc_source_theta(const PcState &S, const double (&cube)[DPL], double (&th)[DPL], int lane, double *ybuf)
{
    const int D = S.D;
#pragma unroll
    for (int k = 0; k < DPL; ++k) if (lane + 64 * k < D) ybuf[lane + 64 * k] = cube[k];
    __syncthreads();                              // one wave per workgroup: cheap
#pragma unroll
    for (int k = 0; k < DPL; ++k)
        th[k] = (lane + 64 * k < D) ? pchip_prior_param(ybuf, lane + 64 * k, D, S.src_data, (long)S.src_ndata) : 0.0;
    __syncthreads();                              // ... before the likelihood re-uses ybuf for theta
}
// S.prior.kind is a kernel argument: the branch is wave-uniform, and a table (kind 2) run of such a handle takes pc_table_theta as ever.
// A source prior has no table: S.prior.lo / .hi are null and nothing is loaded.
template <int DPL, bool AD>
__device__ __forceinline__ void pc_prior_load(const PcState &S, int lane, LaneTable<DPL> &lt)
{
    if (S.prior.kind == 3) {
        lt.mask = 0u;
#pragma unroll
        for (int k = 0; k < DPL; ++k) { lt.type[k] = 0; lt.pos[k] = 0; lt.len[k] = 0; lt.hyp[k] = 0; lt.cnt[k] = -1; lt.lay[k] = -1; lt.p0[k] = 0.0; lt.p1[k] = 0.0; lt.p2[k] = 0.0; }
    } else pc_table_load<DPL, AD>(S, lane, lt);
}
template <int DPL, bool AD>
__device__ __forceinline__ void pc_prior_theta(const PcState &S, const LaneTable<DPL> &lt, const double (&cube)[DPL], double (&th)[DPL], int lane,
                                               double *ybuf)
{
    if (S.prior.kind == 3) pc_source_theta<DPL>(S, cube, th, lane, ybuf);
    else pc_table_theta<DPL, AD>(lt, cube, th, lane, ybuf);
}
#define PC_PRIOR_LOAD(DPL, AD, S, lane, lt) pc_prior_load<DPL, AD>(S, lane, lt)
#define PC_PRIOR_THETA(DPL, AD, S, lt, cube, th, lane, ybuf) pc_prior_theta<DPL, AD>(S, lt, cube, th, lane, ybuf)
#else
#define PC_PRIOR_LOAD(DPL, AD, S, lane, lt) pc_table_load<DPL, AD>(S, lane, lt)
#define PC_PRIOR_THETA(DPL, AD, S, lt, cube, th, lane, ybuf) pc_table_theta<DPL, AD>(lt, cube, th, lane, ybuf)
#endif

#ifdef PCHIP_USER_SOURCE
// the user's function (pc_rtc.hip): its text follows the library's in the run-time unit, so that none of its macros reach these kernels
__device__ double pchip_loglikelihood(const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);
#endif

// The dynamic LDS of a kernel that evaluates the likelihood, as `name`: the declaration every kernel had -- except in the unit of a
// quadratic-form handle (PCHIP_USER_QUAD, below), where the kernel's own layout starts behind that form's residual blocks, and of a
// handle with shared values (PCHIP_USER_SHARED, below), where it starts behind the form's whole front block.
#ifdef PCHIP_USER_SHARED
#define PC_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) char name##_all[]; char *const name = name##_all + PC_FRONT_LDS_BYTES
#elif defined(PCHIP_USER_QUAD)
#define PC_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) char name##_all[]; char *const name = name##_all + PC_QUAD_LDS_BYTES
#else
#define PC_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) char name[]
#endif

template <int DPL, int NROWS>
__device__ __forceinline__ double wsum(double v) { return (DPL > 1) ? wave_sum<4>(v) : wave_sum<NROWS>(v); }

#ifdef PCHIP_USER_SHARED
// Shared values (pchip_source_create_shared; PCHIP_USER_SHARED and PCHIP_SRC_NSHARED in front of the defines of the handle's form): what
// the user's terms need of theta alone -- a table on a grid, spline coefficients, rotated parameters -- is computed ONCE per evaluated
// point, one lane per value, and every function of the form gets the finished block as `shared` behind theta.  The defined order
// (tests/test_source_shared.py rests on it):
//   1. theta to the wave's LDS copy, behind the barrier a source evaluation always had
//   2. lane l: shared[k] = pchip_shared_value(theta, k) for k = l, l + 64, ... -- the returned double stored as it is --; one barrier
//   3. the form as it is without shared values: the strided term loop and wave_sum<4>, or the residual block and the walk over P; finish
// The blocks -- two, for the two ends of a bracket; PC_SHARED_NP doubles each, even, so that they stay on 16 bytes -- lie in the form's
// front block of the dynamic LDS, behind the residual blocks of a quadratic form: block 0 belongs to the theta in ybuf, block 1 to the
// one in ybuf2.  PC_SH_PARAM / PC_SH_PASS / PC_SH_BLOCK(b) put the parameter, the argument and a block's address into the adaptors and
// their calls below; without PCHIP_USER_SHARED they are empty and every token is what it was.
constexpr long PC_SHARED_N = (long)(PCHIP_SRC_NSHARED);
constexpr long PC_SHARED_NP = (PC_SHARED_N + 1) & ~1L;
#ifdef PCHIP_USER_QUAD
#define PC_SHARED_OFF_BYTES (sizeof(double) * 2 * (size_t)((((long)(PCHIP_SRC_NTERMS)) + 1) & ~1L))
#else
#define PC_SHARED_OFF_BYTES ((size_t)0)
#endif
#define PC_FRONT_LDS_BYTES (PC_SHARED_OFF_BYTES + sizeof(double) * 2 * (size_t)PC_SHARED_NP)
__device__ double pchip_shared_value(const double *theta, int nDims, const double *data, long ndata, long k);
__device__ __forceinline__ double *pc_shared_block(int b)
{
    extern __shared__ __attribute__((aligned(16))) char pc_front_all[];      // (the dynamic LDS from its start: every such declaration names it)
    return (double *)(pc_front_all + PC_SHARED_OFF_BYTES) + (size_t)b * PC_SHARED_NP;
}
// step 2 for NP points (theta[p]: their LDS copies, already behind a barrier): block p is theta[p]'s
template <int NP>
__device__ __forceinline__ void pc_shared_fill(const PcState &S, const double *const (&theta)[NP], int lane)
{
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        double *sh = pc_shared_block(p);
        for (long k = lane; k < PC_SHARED_N; k += 64) sh[k] = pchip_shared_value(theta[p], S.D, S.src_data, (long)S.src_ndata, k);
    }
    __syncthreads();                              // one wave per workgroup: cheap
}
#define PC_SH_PARAM , const double *shared
#define PC_SH_PASS , shared
#define PC_SH_BLOCK(b) , pc_shared_block(b)
#else
#define PC_SH_PARAM
#define PC_SH_PASS
#define PC_SH_BLOCK(b)
#endif

#ifdef PCHIP_USER_TERMS
// The terms form of a user source (pchip_source_create_terms; pc_rtc.hip defines PCHIP_USER_TERMS and PCHIP_SRC_NTERMS in front of this
// text in such a handle's unit): the likelihood is finish(sum of PCHIP_SRC_NTERMS terms), and the wavefront SHARES the loop over the
// terms instead of every lane running all of it.  The sum has one defined order (the parity tests rest on it):
//   lane l:  s_l = 0;  for (i = l; i < nterms; i += 64) s_l = s_l + term(i)       -- a plain IEEE add of the returned value
//   wave:    wave_sum<4> of the 64 partials: a balanced pairwise tree over the lanes in lane order within each row of sixteen,
//            then (r0 + r1) + (r2 + r3); a lane without a term contributes 0.0 and takes part in the reduction
// The term's value passes an empty asm before it is added: hipcc contracts by default (-ffp-contract=fast, on whatever the optimiser
// has made of the code), and the add must not fuse with a multiply at the end of the user's inlined term.
// Lane-consecutive i: a data block laid out as a structure of arrays is read with coalesced loads.  No LDS traffic and no barrier in
// the loop (theta is read from the LDS copy behind the one barrier a source evaluation always had).
//
// Several sums per evaluation (pchip_source_create_sums; PCHIP_USER_SUMS and PCHIP_SRC_NSUMS in front as well): ONE call of the user's
// pchip_logl_terms per (point, i) writes the i-th term of every sum, and each sum k on its own is formed exactly as above -- its bits do
// not depend on how many sums travel beside it.  Everything below is written for PC_NSUMS sums; the one-sum form is its length-1 case
// behind two adaptors around the user's pchip_logl_term / pchip_logl_finish.
#ifdef PCHIP_USER_SUMS
constexpr int PC_NSUMS = (int)(PCHIP_SRC_NSUMS);
__device__ void   pchip_logl_terms(const double *theta PC_SH_PARAM, int nDims, const double *data, long ndata, long i, double *t);
__device__ double pchip_logl_finish_sums(const double *sums, const double *theta PC_SH_PARAM, double *phi, int nDims, int nDerived, const double *data, long ndata);
__device__ __forceinline__ void pc_user_terms(const double *theta PC_SH_PARAM, int nDims, const double *data, long ndata, long i, double (&t)[PC_NSUMS])
{
    pchip_logl_terms(theta PC_SH_PASS, nDims, data, ndata, i, t);
}
__device__ __forceinline__ double pc_user_finish(const double *sums, const double *theta PC_SH_PARAM, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    return pchip_logl_finish_sums(sums, theta PC_SH_PASS, phi, nDims, nDerived, data, ndata);
}
#elif defined(PCHIP_USER_QUAD)
// The quadratic form (pchip_source_create_quad; PCHIP_USER_QUAD in front as well, PCHIP_SRC_NTERMS = nres): a Gaussian in data space with a
// dense precision matrix, chi2 = r^T P r, where the user's pchip_residual supplies r_i and P (nres x nres, row-major, exactly as given)
// lies behind the user's data in the run's block, at S.src_data + S.src_ndata.  To everything below it is a terms handle of one sum: the
// finished chi2 is `the sum`.  Its one defined order (tests/test_source_quad.py rests on it):
//   1. lane l: r_i = pchip_residual(i) for i = l, l + 64, ... into a block of nres doubles in LDS; one barrier
//   2. lane l, every column j = l, l + 64, ...: q_j = 0.0; for (i = 0; i < nres; ++i) q_j = fma(P[i * nres + j], r_i, q_j)
//      -- the fused multiply-add is explicit and correctly rounded; the 64 lanes read 64 consecutive doubles of row i, r_i is an LDS broadcast
//   3. t_j = r_j * q_j, one IEEE multiply, kept from fusing with the add behind it by the empty asm of the terms form
//   4. chi2 = the sum of the t_j in the terms form's order: lane l adds t_l, t_(l + 64), ... to 0.0, then wave_sum<4>
// The residual blocks -- two, for the two ends of a bracket -- are the FIRST 2 x PC_QUAD_NP doubles of the workgroup's dynamic LDS: every
// kernel that evaluates the likelihood starts its own layout behind them (PC_DYN_LDS above; the launchers add them: pc_quad_lds, inside pc_front_lds), so that
// the evaluation code finds them without a pointer handed down through every caller.  One wavefront a workgroup, as for every source.
constexpr int PC_NSUMS = 1;
constexpr long PC_QUAD_N = (long)(PCHIP_SRC_NTERMS);
constexpr long PC_QUAD_NP = (PC_QUAD_N + 1) & ~1L;       // a block's length in doubles: even, both blocks on 16 bytes for the paired reads
#define PC_QUAD_LDS_BYTES (sizeof(double) * 2 * (size_t)PC_QUAD_NP)
__device__ double pchip_residual(const double *theta PC_SH_PARAM, int nDims, const double *data, long ndata, long i);
__device__ double pchip_logl_finish(double chi2, const double *theta PC_SH_PARAM, double *phi, int nDims, int nDerived, const double *data, long ndata);
__device__ __forceinline__ double pc_user_finish(const double *sums, const double *theta PC_SH_PARAM, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    return pchip_logl_finish(sums[0], theta PC_SH_PASS, phi, nDims, nDerived, data, ndata);
}
#else
constexpr int PC_NSUMS = 1;
__device__ double pchip_logl_term(const double *theta PC_SH_PARAM, int nDims, const double *data, long ndata, long i);
__device__ double pchip_logl_finish(double sum, const double *theta PC_SH_PARAM, double *phi, int nDims, int nDerived, const double *data, long ndata);
__device__ __forceinline__ void pc_user_terms(const double *theta PC_SH_PARAM, int nDims, const double *data, long ndata, long i, double (&t)[PC_NSUMS])
{
    t[0] = pchip_logl_term(theta PC_SH_PASS, nDims, data, ndata, i);
}
__device__ __forceinline__ double pc_user_finish(const double *sums, const double *theta PC_SH_PARAM, double *phi, int nDims, int nDerived, const double *data, long ndata)
{
    return pchip_logl_finish(sums[0], theta PC_SH_PASS, phi, nDims, nDerived, data, ndata);
}
#endif
#ifdef PCHIP_USER_QUAD
// rows of P a lane keeps in flight for every column it holds, and the columns (strips of 64) it walks side by side: the fused multiply-adds
// of one column are a dependent chain, the strips' chains are independent and share every r_i read.  Eight loads in flight a lane, two
// chains for one point and four for a pair (with four strips, sixteen loads, the prior-table variants of k_slice spilled 28 vector
// registers; with two none does)
constexpr int PC_QUAD_FLIGHT = 4;
constexpr int PC_QUAD_STRIPS = 2;
__device__ __forceinline__ double *pc_quad_blocks()
{
    extern __shared__ __attribute__((aligned(16))) char pc_quad_res[];       // (the dynamic LDS from its start: every such declaration names it)
    return (double *)pc_quad_res;
}
// G strips of columns from column j0 on, NP points: q of every (column, point) in the defined order, then the products and the lane's adds in
// ascending j.  A lane whose column lies beyond nres walks column 0 (an address inside the matrix, no divergence) and adds nothing.
template <int NP, int G>
__device__ __forceinline__ void pc_quad_strips(const double *__restrict__ P, const double *r, long j0, int lane, double (&s)[NP])
{
    typedef double v2d __attribute__((ext_vector_type(2)));
    constexpr long N = PC_QUAD_N;
    constexpr int U = PC_QUAD_FLIGHT;
    double q[G][NP];
    const double *col[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const long j = j0 + 64 * g + lane;
        col[g] = P + (j < N ? j : 0);
#pragma unroll
        for (int p = 0; p < NP; ++p) q[g][p] = 0.0;
    }
    long i = 0;
    for (; i + U <= N; i += U) {                                  // (i a multiple of four: r + i on 16 bytes)
        double m[U][G];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) m[u][g] = col[g][(size_t)(i + u) * N];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int u = 0; u < U; u += 2) {
                const v2d rr = *(const v2d *)(r + p * PC_QUAD_NP + i + u);
#pragma unroll
                for (int g = 0; g < G; ++g) q[g][p] = __builtin_fma(m[u][g], rr.x, q[g][p]);
#pragma unroll
                for (int g = 0; g < G; ++g) q[g][p] = __builtin_fma(m[u + 1][g], rr.y, q[g][p]);
            }
        }
    }
    for (; i < N; ++i) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double m = col[g][(size_t)i * N];
#pragma unroll
            for (int p = 0; p < NP; ++p) q[g][p] = __builtin_fma(m, r[p * PC_QUAD_NP + i], q[g][p]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const long j = j0 + 64 * g + lane;
        if (j < N) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                double t = r[p * PC_QUAD_NP + j] * q[g][p];
                asm volatile("" : "+v"(t));
                s[p] = s[p] + t;
            }
        }
    }
}
// chi2 of NP points (theta[p]: their LDS copies) in ONE walk over P, an accumulator per point and column: a point's bits do not depend on
// whether it was evaluated alone or as one end of a bracket.  No barrier inside the walk.
template <int NP>
__device__ __forceinline__ void pc_quad_sum(const PcState &S, const double *const (&theta)[NP], int lane, double (&chi2)[NP])
{
    constexpr long N = PC_QUAD_N;
    constexpr int G = PC_QUAD_STRIPS;
    constexpr long K = (N + 63) / 64, KF = K / G;                 // strips; whole groups of G
    constexpr int KR = (int)(K % G);                              // ... and the strips of the last group
    double *r = pc_quad_blocks();
#pragma unroll
    for (int p = 0; p < NP; ++p)
        for (long i = lane; i < N; i += 64) r[p * PC_QUAD_NP + i] = pchip_residual(theta[p] PC_SH_BLOCK(p), S.D, S.src_data, (long)S.src_ndata, i);
    __syncthreads();                              // one wave per workgroup: cheap
    const double *P = S.src_data + S.src_ndata;
    double s[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) s[p] = 0.0;
    for (long k = 0; k < KF; ++k) pc_quad_strips<NP, G>(P, r, 64 * G * k, lane, s);
    if constexpr (KR > 0) pc_quad_strips<NP, (KR > 0 ? KR : 1)>(P, r, 64 * G * KF, lane, s);
#pragma unroll
    for (int p = 0; p < NP; ++p) chi2[p] = wave_sum<4>(s[p]);
}
__device__ __forceinline__ void pc_terms_sum(const PcState &S, const double *theta, int lane, double (&sum)[PC_NSUMS])
{
    const double *const th[1] = { theta };
    pc_quad_sum<1>(S, th, lane, sum);
}
__device__ __forceinline__ void pc_terms_sum2(const PcState &S, const double *thA, const double *thB, int lane, double (&sA)[PC_NSUMS],
                                              double (&sB)[PC_NSUMS])
{
    const double *const th[2] = { thA, thB };
    double c[2];
    pc_quad_sum<2>(S, th, lane, c);
    sA[0] = c[0]; sB[0] = c[1];
}
#else
// terms a lane keeps in flight -- their loads travel together, a lane's wait for the data is what a short term costs --: four for one sum
// (two a point in the pair pass), fewer as the sums multiply the values held (PC_NSUMS of them a term and point, beside as many accumulators)
constexpr int PC_TERMS_FLIGHT = PC_NSUMS <= 1 ? 4 : (PC_NSUMS <= 4 ? 2 : 1);
constexpr int PC_TERMS_FLIGHT2 = PC_NSUMS <= 1 ? 2 : 1;

// (the adds of a sum one after the other in the order of i)
__device__ __forceinline__ void pc_terms_sum(const PcState &S, const double *theta, int lane, double (&sum)[PC_NSUMS])
{
    constexpr long N = (long)(PCHIP_SRC_NTERMS);
    constexpr int U = PC_TERMS_FLIGHT;
    double s[PC_NSUMS];
#pragma unroll
    for (int k = 0; k < PC_NSUMS; ++k) s[k] = 0.0;
    long i = lane;
    if constexpr (U > 1) {
        for (; i + 64 * (U - 1) < N; i += 64 * U) {
            double t[U][PC_NSUMS];
#pragma unroll
            for (int u = 0; u < U; ++u) pc_user_terms(theta PC_SH_BLOCK(0), S.D, S.src_data, (long)S.src_ndata, i + 64 * u, t[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < PC_NSUMS; ++k) { asm volatile("" : "+v"(t[u][k])); s[k] = s[k] + t[u][k]; }
        }
    }
    for (; i < N; i += 64) {
        double t[PC_NSUMS];
        pc_user_terms(theta PC_SH_BLOCK(0), S.D, S.src_data, (long)S.src_ndata, i, t);
#pragma unroll
        for (int k = 0; k < PC_NSUMS; ++k) { asm volatile("" : "+v"(t[k])); s[k] = s[k] + t[k]; }
    }
#pragma unroll
    for (int k = 0; k < PC_NSUMS; ++k) sum[k] = wave_sum<4>(s[k]);
}
// two points in ONE pass over the data, PC_NSUMS accumulators each: every sum in the order above, so its bits do not depend on whether the
// point was evaluated alone or in a pair
__device__ __forceinline__ void pc_terms_sum2(const PcState &S, const double *thA, const double *thB, int lane, double (&sA)[PC_NSUMS],
                                              double (&sB)[PC_NSUMS])
{
    constexpr long N = (long)(PCHIP_SRC_NTERMS);
    constexpr int U = PC_TERMS_FLIGHT2;
    double a[PC_NSUMS], b[PC_NSUMS];
#pragma unroll
    for (int k = 0; k < PC_NSUMS; ++k) { a[k] = 0.0; b[k] = 0.0; }
    long i = lane;
    if constexpr (U > 1) {
        for (; i + 64 * (U - 1) < N; i += 64 * U) {
            double tA[U][PC_NSUMS], tB[U][PC_NSUMS];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pc_user_terms(thA PC_SH_BLOCK(0), S.D, S.src_data, (long)S.src_ndata, i + 64 * u, tA[u]);
                pc_user_terms(thB PC_SH_BLOCK(1), S.D, S.src_data, (long)S.src_ndata, i + 64 * u, tB[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < PC_NSUMS; ++k) {
                    asm volatile("" : "+v"(tA[u][k])); asm volatile("" : "+v"(tB[u][k]));
                    a[k] = a[k] + tA[u][k]; b[k] = b[k] + tB[u][k];
                }
        }
    }
    for (; i < N; i += 64) {
        double tA[PC_NSUMS], tB[PC_NSUMS];
        pc_user_terms(thA PC_SH_BLOCK(0), S.D, S.src_data, (long)S.src_ndata, i, tA);
        pc_user_terms(thB PC_SH_BLOCK(1), S.D, S.src_data, (long)S.src_ndata, i, tB);
#pragma unroll
        for (int k = 0; k < PC_NSUMS; ++k) {
            asm volatile("" : "+v"(tA[k])); asm volatile("" : "+v"(tB[k]));
            a[k] = a[k] + tA[k]; b[k] = b[k] + tB[k];
        }
    }
#pragma unroll
    for (int k = 0; k < PC_NSUMS; ++k) { sA[k] = wave_sum<4>(a[k]); sB[k] = wave_sum<4>(b[k]); }
}
#endif
// logL of theta (uniform over the wave) and, in `sum`, the finished sums it came from: whoever accepts the point keeps them, and the
// derived parameters are finish(sums, theta) again -- never a second walk over the data
template <int DPL>
__device__ __forceinline__ double like_eval_terms(const PcState &S, const double (&th)[DPL], const LaneDims<DPL> &ld, int lane, double *ybuf,
                                                  double (&sum)[PC_NSUMS])
{
#pragma unroll
    for (int k = 0; k < DPL; ++k) if (ld.on[k]) ybuf[lane + 64 * k] = th[k];
    __syncthreads();                              // one wave per workgroup: cheap
#ifdef PCHIP_USER_SHARED
    { const double *const one[1] = { ybuf }; pc_shared_fill<1>(S, one, lane); }
#endif
    pc_terms_sum(S, ybuf, lane, sum);
    double phi[PC_SRC_MAX_DERIVED];
    const double l = pc_user_finish(sum, ybuf PC_SH_BLOCK(0), phi, S.D, S.nDer, S.src_data, (long)S.src_ndata);
    __syncthreads();
    return l;
}
// all nDerived values of an accepted point from its sums (lane 0 writes them to out)
template <int DPL>
__device__ __forceinline__ void like_phi_terms(const PcState &S, const double (&th)[DPL], const LaneDims<DPL> &ld, int lane, double *ybuf,
                                               const double (&sum)[PC_NSUMS], double *out)
{
#pragma unroll
    for (int k = 0; k < DPL; ++k) if (ld.on[k]) ybuf[lane + 64 * k] = th[k];
    __syncthreads();
#ifdef PCHIP_USER_SHARED        // (an accepted point keeps its sums, not its shared values: step 2 again)
    { const double *const one[1] = { ybuf }; pc_shared_fill<1>(S, one, lane); }
#endif
    double phi[PC_SRC_MAX_DERIVED];
    (void)pc_user_finish(sum, ybuf PC_SH_BLOCK(0), phi, S.D, S.nDer, S.src_data, (long)S.src_ndata);
    if (lane == 0) for (int e = 0; e < S.nDer; ++e) out[e] = phi[e];
    __syncthreads();
}
#endif

// returns logL of theta (uniform over the wave).  ybuf: per-wave LDS scratch of >= D doubles.
// (KIND >= 0: the likelihood is known when the kernel is compiled -- k_slice's LEAN variants -- and the other branches are not there)
template <int DPL, int NROWS, int KIND = -1>
__device__ __forceinline__ double like_eval(const PcState &S, const double (&th)[DPL], const LaneDims<DPL> &ld,
                                            int lane, double *ybuf)
{
    const int D = S.D;
    const PcLike &L = S.like;
    const int kind = KIND >= 0 ? KIND : L.kind;
    if (kind == PC_LIKE_GAUSSIAN) {            // gaussian.f90:25-34
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (ld.on[k]) { const double z = (th[k] - L.mu) * L.inv_sigma; s += z * z; }
        s = wsum<DPL, NROWS>(s);
        return L.norm - s / 2.0;
    } else if (kind == PC_LIKE_RASTRIGIN) {    // rastrigin.f90:33
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DPL; ++k)
            if (ld.on[k]) s += 8.515435146961291 /* log(4991.21750) */ + th[k] * th[k] - 10.0 * cos(PC_TWO_PI * th[k]);
        s = wsum<DPL, NROWS>(s);
        return -s;
    } else if (kind == PC_LIKE_TWIN_GAUSSIAN) {  // twin_gaussian.f90:29-46
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < DPL; ++k)
            if (ld.on[k]) {
                const int dim = lane + 64 * k;
                const double m1 = dim < 2 ? -0.5 : 0.0, m2 = dim < 2 ? 0.5 : 0.0;
                const double z1 = (th[k] - m1) * L.inv_sigma, z2 = (th[k] - m2) * L.inv_sigma;
                s1 += z1 * z1; s2 += z2 * z2;
            }
        s1 = wsum<DPL, NROWS>(s1); s2 = wsum<DPL, NROWS>(s2);
        return pc_logaddexp(L.norm - s1 / 2.0, L.norm - s2 / 2.0) - 0.6931471805599453;
#ifdef PCHIP_USER_TERMS
    } else if (kind == PC_LIKE_SOURCE) {          // the terms form: the wave shares the loop over the terms (like_eval_terms)
        double sum[PC_NSUMS];
        return like_eval_terms<DPL>(S, th, ld, lane, ybuf, sum);
#elif defined(PCHIP_USER_SOURCE)
    } else if (kind == PC_LIKE_SOURCE) {          // the user's function (pc_rtc.hip): every lane evaluates it on the same LDS copy of theta,
#pragma unroll                                    // so the result is wave-uniform without a broadcast
        for (int k = 0; k < DPL; ++k) if (ld.on[k]) ybuf[lane + 64 * k] = th[k];
        __syncthreads();                          // one wave per workgroup: cheap
        double phi[PC_SRC_MAX_DERIVED];
        const double l = pchip_loglikelihood(ybuf, phi, D, S.nDer, S.src_data, (long)S.src_ndata);
        __syncthreads();
        return l;
#endif
    } else {                                      // random_gaussian.f90:17-30, utils.F90:1028-1048
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (ld.on[k]) ybuf[lane + 64 * k] = th[k] - ld.mean[k];
        __syncthreads();                          // one wave per workgroup: cheap
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < DPL; ++k)
            if (ld.on[k]) {
                const int a = lane + 64 * k;
                double t = 0.0;
                // invcov is uploaded TRANSPOSED so that lanes read consecutive addresses
                for (int b = 0; b < D; ++b) t += L.invcov[(size_t)b * D + a] * ybuf[b];
                q += (th[k] - ld.mean[k]) * t;
            }
        q = wsum<DPL, NROWS>(q);
        __syncthreads();
        return -((double)D * PC_LOG_TWO_PI + L.logdetcov) / 2.0 - q / 2.0;
    }
}

// derived parameters of an accepted point (lane-uniform results)
template <int DPL, int NROWS, int KIND = -1>
__device__ __forceinline__ void like_phi(const PcState &S, const double (&th)[DPL], const LaneDims<DPL> &ld,
                                         int lane, double &phi0, double &phi1)
{
    phi0 = 0.0; phi1 = 0.0;
    if (S.nDer == 0) return;
    const int kind = KIND >= 0 ? KIND : S.like.kind;
    if (kind == PC_LIKE_GAUSSIAN) {        // gaussian.f90:36-37
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (ld.on[k]) r2 += (th[k] - S.like.mu) * (th[k] - S.like.mu);
        r2 = wsum<DPL, NROWS>(r2);
        phi0 = sqrt(r2);
        if (S.nDer >= 2) phi1 = pc_log_ball(phi0, S.D, S.like.log_vn);
    } else if (kind == PC_LIKE_TWIN_GAUSSIAN) {   // twin_gaussian.f90:48-52
        const double t0 = readlane_f64(th[0], 0);
        phi0 = (t0 > 0.5) ? 1.0 : -1.0;
    }
}

#ifdef PCHIP_USER_SOURCE
// all nDerived values of an accepted point of a source likelihood (the user's function once more; lane 0 writes them to out)
template <int DPL>
__device__ __forceinline__ void like_phi_source(const PcState &S, const double (&th)[DPL], const LaneDims<DPL> &ld, int lane, double *ybuf,
                                                double *out)
{
#pragma unroll
    for (int k = 0; k < DPL; ++k) if (ld.on[k]) ybuf[lane + 64 * k] = th[k];
    __syncthreads();
    double phi[PC_SRC_MAX_DERIVED];
    (void)pchip_loglikelihood(ybuf, phi, S.D, S.nDer, S.src_data, (long)S.src_ndata);
    if (lane == 0) for (int e = 0; e < S.nDer; ++e) out[e] = phi[e];
    __syncthreads();
}
#endif

// ------------------------------------------------------------------------------------------
// initial live points: GenerateLivePoints, linear mode (generate.F90:150-183)
// one wave per attempt; attempts are the oracle's PC_DOM_LIVEGEN streams.
// ------------------------------------------------------------------------------------------
// PT = 1: the prior is a table (pc_table_theta); PT = 0, the default, is the uniform box
template <int DPL, int PT = 0>
__global__ __launch_bounds__(64) void k_generate_live(PcState S, int attempt0, double *rows /* [n][nT] */,
                                                     double *rows_logL)
{
    PC_DYN_LDS(smem);
    double *ybuf = (double *)smem;
    const int lane = threadIdx.x, a = blockIdx.x, attempt = attempt0 + a;
    const int D = S.D, nT = S.nT;
    LaneDims<DPL> ld;
    double cube[DPL], th[DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        const int dim = lane + 64 * k;
        ld.on[k] = dim < D;
        const double lo = (PT == 0 && ld.on[k] && S.prior.lo) ? S.prior.lo[dim] : 0.0;
        const double hi = (PT == 0 && ld.on[k] && S.prior.hi) ? S.prior.hi[dim] : 1.0;
        ld.lo[k] = lo; ld.span[k] = hi - lo;
        ld.mean[k] = (ld.on[k] && S.like.mean) ? S.like.mean[dim] : 0.0;
        cube[k] = !ld.on[k] ? 0.5 : (S.seq_mode ? pc_seq_uniform(S, (unsigned long long)attempt * D + dim)
                                                 : pc_uniform(S.k0, S.k1, PC_DOM_LIVEGEN, 0u, (uint32_t)attempt, (uint32_t)dim));
        th[k] = pc_box_theta(ld.lo[k], ld.span[k], cube[k]);
    }
    if constexpr (PT != 0) {
        LaneTable<DPL> lt;
        PC_PRIOR_LOAD(DPL, true, S, lane, lt);
        PC_PRIOR_THETA(DPL, true, S, lt, cube, th, lane, ybuf);
    }
#ifdef PCHIP_USER_TERMS
    double tsum[PC_NSUMS] = {};
    const double logL = S.like.kind == PC_LIKE_SOURCE ? like_eval_terms<DPL>(S, th, ld, lane, ybuf, tsum) : like_eval<DPL, 4>(S, th, ld, lane, ybuf);
#else
    const double logL = like_eval<DPL, 4>(S, th, ld, lane, ybuf);
#endif
    double phi0, phi1;
    like_phi<DPL, 4>(S, th, ld, lane, phi0, phi1);
    double *row = rows + (size_t)a * nT;
#ifdef PCHIP_USER_TERMS
    if (S.like.kind == PC_LIKE_SOURCE && S.nDer > 0) like_phi_terms<DPL>(S, th, ld, lane, ybuf, tsum, row + S.d0);
#elif defined(PCHIP_USER_SOURCE)
    if (S.like.kind == PC_LIKE_SOURCE && S.nDer > 0) like_phi_source<DPL>(S, th, ld, lane, ybuf, row + S.d0);
#endif
#pragma unroll
    for (int k = 0; k < DPL; ++k)
        if (ld.on[k]) { row[lane + 64 * k] = cube[k]; row[S.p0 + lane + 64 * k] = th[k]; }
    if (lane == 0) {
        if (S.like.kind != PC_LIKE_SOURCE) {
            if (S.nDer >= 1) row[S.d0] = phi0;
            if (S.nDer >= 2) row[S.d0 + 1] = phi1;
            for (int e = 2; e < S.nDer; ++e) row[S.d0 + e] = 0.0;
        }
        row[S.b0] = S.logzero;                   // generate.F90:163
        row[S.l0] = logL;
        rows_logL[a] = logL;
    }
}

// the device transform of a prior table alone (pchip_prior_transform: parity tests against the host function): one wave a point.
// The device batch callback's prior as well (pc_park.hip's blocks): a table, or the uniform box (S.prior.kind == 1, wave-uniform).
template <int DPL>
__global__ __launch_bounds__(64) void k_prior_transform(PcState S, const double *cubes /* [n][D] */, double *thetas /* [n][D] */)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *ybuf = (double *)smem;
    const int lane = threadIdx.x, D = S.D;
    const size_t base = (size_t)blockIdx.x * D;
    if (S.prior.kind == 1) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const int dim = lane + 64 * k;
            if (dim >= D) continue;
            const double lo = S.prior.lo ? S.prior.lo[dim] : 0.0, hi = S.prior.hi ? S.prior.hi[dim] : 1.0;
            thetas[base + dim] = pc_box_theta(lo, hi - lo, cubes[base + dim]);
        }
        return;
    }
    LaneTable<DPL> lt;
    PC_PRIOR_LOAD(DPL, true, S, lane, lt);
    double cube[DPL], th[DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) cube[k] = (lane + 64 * k < D) ? cubes[base + lane + 64 * k] : 0.5;
    PC_PRIOR_THETA(DPL, true, S, lt, cube, th, lane, ybuf);
#pragma unroll
    for (int k = 0; k < DPL; ++k) if (lane + 64 * k < D) thetas[base + lane + 64 * k] = th[k];
}

#ifdef PCHIP_USER_SOURCE
// a source likelihood alone (pchip_source_eval: tests, and users checking their source): one wave a point, through the evaluation code of
// the sampling kernels -- like_eval and the derived parameters as k_generate_live writes them -- for both forms of source
template <int DPL>
__global__ __launch_bounds__(64) void k_source_eval(PcState S, const double *thetas /* [n][D] */, double *logL /* [n] */, double *phi /* [n][nDer] */)
{
    PC_DYN_LDS(smem);
    double *ybuf = (double *)smem;
    const int lane = threadIdx.x, D = S.D;
    const size_t base = (size_t)blockIdx.x * D;
    LaneDims<DPL> ld;
    double th[DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        ld.on[k] = lane + 64 * k < D;
        ld.lo[k] = 0.0; ld.span[k] = 1.0; ld.mean[k] = 0.0;
        th[k] = ld.on[k] ? thetas[base + lane + 64 * k] : 0.0;
    }
    double *out = phi + (size_t)blockIdx.x * S.nDer;
#ifdef PCHIP_USER_TERMS
    double sum[PC_NSUMS];
    const double l = like_eval_terms<DPL>(S, th, ld, lane, ybuf, sum);
    if (S.nDer > 0) like_phi_terms<DPL>(S, th, ld, lane, ybuf, sum, out);
#else
    const double l = like_eval<DPL, 4>(S, th, ld, lane, ybuf);
    if (S.nDer > 0) like_phi_source<DPL>(S, th, ld, lane, ybuf, out);
#endif
    if (lane == 0) logL[blockIdx.x] = l;
}
#endif

#ifdef PCHIP_USER_QUAD_BATCH
// The batched quadratic form (pchip_source_create_quad_batch; pc_rtc.hip puts PCHIP_USER_QUAD_BATCH and PCHIP_SRC_NRES in front of this text
// in such a handle's unit, beside PCHIP_USER_SOURCE and nothing else): the handle has NO in-kernel evaluation -- no sampling kernel is ever
// instantiated from its unit -- and the two kernels below are all its module is asked for.  They stand around pc_quad_mm.hip's
// k_quad_chi2_mm, which forms chi2 = r^T P r of all rows of a block on the matrix cores (the contract and the order: there).
__device__ double pchip_residual(const double *theta, int nDims, const double *data, long ndata, long i);
__device__ double pchip_logl_finish(double chi2, const double *theta, double *phi, int nDims, int nDerived, const double *data, long ndata);
// one thread per (row, i), i fastest: R[row][i] = pchip_residual(theta_row, i), the returned double as it is, into a block of leading
// dimension ldr = nres rounded up to 16 and of n rounded up to 64 rows; zeros in the padding columns and the padding rows
__global__ __launch_bounds__(256) void k_quad_residuals(PcState S, int n, const double *thetas /* [n][D] */, double *R /* [rows][ldr] */)
{
    constexpr long N = (long)(PCHIP_SRC_NRES), LDR = (N + 15) & ~15L;
    const long rows = ((long)n + 63) / 64 * 64;
    const long cell = (long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= rows * LDR) return;
    const long row = cell / LDR, i = cell - row * LDR;
    R[cell] = (row < n && i < N) ? pchip_residual(thetas + (size_t)row * S.D, S.D, S.src_data, (long)S.src_ndata, i) : 0.0;
}
// one thread per row: chi2 = the row's ncb partials added to 0.0 in ascending order, logL = pchip_logl_finish(chi2, theta_row, ...), the
// derived parameters it wrote to phi[row][nDer]
__global__ __launch_bounds__(64) void k_quad_finish(PcState S, int n, const double *thetas /* [n][D] */, const double *part /* [rows][ncb] */, int ncb,
                                                    double *logL /* [n] */, double *phi /* [n][nDer] */)
{
    const long row = (long)blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;
    double chi2 = 0.0;
    for (int c = 0; c < ncb; ++c) chi2 = chi2 + part[(size_t)row * ncb + c];
    double ph[PC_SRC_MAX_DERIVED];
    const double l = pchip_logl_finish(chi2, thetas + (size_t)row * S.D, ph, S.D, S.nDer, S.src_data, (long)S.src_ndata);
    for (int e = 0; e < S.nDer; ++e) phi[(size_t)row * S.nDer + e] = ph[e];
    logL[row] = l;
}
#endif

// ------------------------------------------------------------------------------------------
// The device maximiser (pchip_maximise_device): `maximise = T` for a problem that lives wholly on the device.  Restates dXdtheta
// (maximiser.F90:179-207), nelder_mead (nelder_mead.f90:7-83) and calculate_point (calculate.f90:6-50) as pc_maximise.hip does on the
// host, one wavefront a problem, lane = coordinate (nDims <= 64), through the evaluation code above: PC_PRIOR_THETA, like_eval.
// Every decision is taken on a value read from lane 0, so control flow and the barriers inside the evaluation stay wave-uniform.
// ------------------------------------------------------------------------------------------
// LDS of k_maximise in doubles: ybuf [D], simplex [D + 1][D], values [D + 1], one D x D matrix, the order [D + 1] (ints)
#define PC_MAX_LDS_DOUBLES(D) ((size_t)(D) + (size_t)((D) + 1) * (D) + ((D) + 1) + (size_t)(D) * (D) + ((D) + 2) / 2)

template <int DPL>
__device__ __forceinline__ void pc_max_lanes(const PcState &S, int lane, LaneDims<DPL> &ld, LaneTable<DPL> &lt, double *ybuf)
{
    static_assert(DPL == 1, "the maximiser holds one coordinate a lane: nDims <= 64");
    const bool box = S.prior.kind < 2;
    ld.on[0] = lane < S.D;
    const double lo = (box && ld.on[0] && S.prior.lo) ? S.prior.lo[lane] : 0.0;
    const double hi = (box && ld.on[0] && S.prior.hi) ? S.prior.hi[lane] : 1.0;
    ld.lo[0] = lo; ld.span[0] = hi - lo;
    ld.mean[0] = (ld.on[0] && S.like.mean) ? S.like.mean[lane] : 0.0;
    if (!box) PC_PRIOR_LOAD(DPL, true, S, lane, lt);
    else { lt.mask = 0u; lt.type[0] = 0; lt.pos[0] = 0; lt.len[0] = 0; lt.hyp[0] = 0; lt.cnt[0] = -1; lt.lay[0] = -1; lt.p0[0] = 0.0; lt.p1[0] = 0.0; lt.p2[0] = 0.0; }
}
// cube -> theta: the table or the source prior of the sampling kernels, else the box as k_generate_live forms it
template <int DPL>
__device__ __forceinline__ void pc_max_theta(const PcState &S, const LaneDims<DPL> &ld, const LaneTable<DPL> &lt, const double (&cube)[DPL],
                                             double (&th)[DPL], int lane, double *ybuf)
{
    if (S.prior.kind >= 2) PC_PRIOR_THETA(DPL, true, S, lt, cube, th, lane, ybuf);
    else th[0] = pc_box_theta(ld.lo[0], ld.span[0], cube[0]);
}
// determinant of the column-major n x n matrix in LDS (destroyed): det_cm's elimination order (pc_maximise.hip, nelder_mead.f90:168-209), row
// swaps on a zero pivot included; lane = row.  The caller's stores to M need no barrier of their own.
__device__ inline double pc_max_det(double *M, int n, int lane)
{
    __syncthreads();
    int sign = 1;
    for (int k = 0; k < n - 1; ++k) {
        double pkk = readlane_f64(M[k * n + k], 0);
        if (pkk == 0.0) {
            const unsigned long long nz = pc_lanes(lane > k && lane < n && M[k * n + lane] != 0.0);
            if (nz == 0ull) return 0.0;
            const int i = __builtin_ctzll(nz);
            if (lane < n) { const double a = M[lane * n + i], b = M[lane * n + k]; M[lane * n + i] = b; M[lane * n + k] = a; }   // lane = column
            sign = -sign;
            __syncthreads();
            pkk = readlane_f64(M[k * n + k], 0);
        }
        if (lane > k && lane < n) {
            const double m = M[k * n + lane] / pkk;
            int i = k + 1;
            for (; i + 3 < n; i += 4) {                // (four columns a step, their loads in flight together: every element the same one operation)
                double a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { a[u] = M[(i + u) * n + lane]; b[u] = M[(i + u) * n + k]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) M[(i + u) * n + lane] = a[u] - m * b[u];
            }
            for (; i < n; ++i) M[i * n + lane] -= m * M[i * n + k];
        }
        __syncthreads();
    }
    double d = sign;
    for (int i = 0; i < n; ++i) d *= M[i * n + i];
    return readlane_f64(d, 0);
}
// log of the prior density in theta at `cube` up to the cube's own (maximiser.F90:179-207): the prior at cube and at D perturbed cubes
// (dx = 1e-5; a step backwards and a flipped sign at the upper edge), the Jacobian in M, its determinant
template <int DPL>
__device__ inline double pc_max_dxdtheta(const PcState &S, const LaneDims<DPL> &ld, const LaneTable<DPL> &lt, const double (&cube)[DPL], int lane,
                                         double *ybuf, double *M)
{
    const int D = S.D;
    const double dx = 1e-5;
    double t0[DPL], t1[DPL], c0[DPL];
    pc_max_theta<DPL>(S, ld, lt, cube, t0, lane, ybuf);
    int s = 1;
    for (int i = 0; i < D; ++i) {
        const bool back = readlane_f64(cube[0], i) + dx >= 1.0;
        c0[0] = cube[0];
        if (lane == i) c0[0] = back ? cube[0] - dx : cube[0] + dx;
        if (back) s = -s;
        pc_max_theta<DPL>(S, ld, lt, c0, t1, lane, ybuf);
        if (lane < D) M[i * D + lane] = t1[0] - t0[0];
    }
    const double det = pc_max_det(M, D, lane);
    return (double)D * log(dx) - log((double)s * det);
}

// candidate values of the posterior leg (maximiser.F90:92-161): logL_i + dXdtheta(cube_i), one wavefront a live row
template <int DPL>
__global__ __launch_bounds__(64) void k_max_rank(PcState S, const double *rows /* [n][nT] */, double *val /* [n] */)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *ybuf = (double *)smem, *M = ybuf + S.D;
    const int lane = threadIdx.x;
    const double *row = rows + (size_t)blockIdx.x * S.nT;
    LaneDims<DPL> ld; LaneTable<DPL> lt;
    pc_max_lanes<DPL>(S, lane, ld, lt, ybuf);
    double cube[DPL];
    cube[0] = ld.on[0] ? row[lane] : 0.5;
    const double dX = pc_max_dxdtheta<DPL>(S, ld, lt, cube, lane, ybuf, M);
    if (lane == 0) val[blockIdx.x] = row[S.l0] + dX;
}

// maximisation_func (maximiser.F90:163-177) behind calculate_point: a point outside the unit cube is logzero without a likelihood call
template <int DPL>
__device__ inline double pc_max_func(const PcState &S, const LaneDims<DPL> &ld, const LaneTable<DPL> &lt, const double (&x)[DPL], int lane,
                                     double *ybuf, double *M, int leg, long long &neval)
{
    if (pc_lanes(ld.on[0] && !(x[0] >= 0.0 && x[0] <= 1.0)) != 0ull) return S.logzero;
    double th[DPL];
    pc_max_theta<DPL>(S, ld, lt, x, th, lane, ybuf);
    double v = readlane_f64(like_eval<DPL, 4>(S, th, ld, lane, ybuf), 0);
    ++neval;
    if (leg == 1 && v > S.logzero) v += pc_max_dxdtheta<DPL>(S, ld, lt, x, lane, ybuf, M);
    return isfinite(v) ? v : S.logzero;          // a source may return NaN: the order of the vertices stays total (pc_max_sort)
}
// the likelihood call of calculate_point (calculate.f90:40-44): logL of theta (uniform over the wave) and, in phi[0 .. nDer), the derived
// parameters by the form's own path, as k_generate_live writes a row
template <int DPL>
__device__ inline double pc_max_point(const PcState &S, const LaneDims<DPL> &ld, const double (&th)[DPL], int lane, double *ybuf, double *phi)
{
#ifdef PCHIP_USER_TERMS
    double tsum[PC_NSUMS] = {};
    double logL = S.like.kind == PC_LIKE_SOURCE ? like_eval_terms<DPL>(S, th, ld, lane, ybuf, tsum) : like_eval<DPL, 4>(S, th, ld, lane, ybuf);
#else
    double logL = like_eval<DPL, 4>(S, th, ld, lane, ybuf);
#endif
    logL = readlane_f64(logL, 0);
    double phi0, phi1;
    like_phi<DPL, 4>(S, th, ld, lane, phi0, phi1);
#ifdef PCHIP_USER_TERMS
    if (S.like.kind == PC_LIKE_SOURCE && S.nDer > 0) like_phi_terms<DPL>(S, th, ld, lane, ybuf, tsum, phi);
#elif defined(PCHIP_USER_SOURCE)
    if (S.like.kind == PC_LIKE_SOURCE && S.nDer > 0) like_phi_source<DPL>(S, th, ld, lane, ybuf, phi);
#endif
    if (lane == 0 && S.like.kind != PC_LIKE_SOURCE) {
        if (S.nDer >= 1) phi[0] = phi0;
        if (S.nDer >= 2) phi[1] = phi1;
    }
    return logL;
}
// the order of the values: stable, ascending (idx[0] worst, idx[nv - 1] best), rank by counting
__device__ __forceinline__ void pc_max_sort(const double *F, int *idx, int nv, int lane)
{
    __syncthreads();
    for (int v = lane; v < nv; v += 64) {
        const double fv = F[v];
        int r = 0;
        for (int u = 0; u < nv; ++u) { const double fu = F[u]; r += (fu < fv || (fu == fv && u < v)) ? 1 : 0; }
        idx[r] = v;
    }
    __syncthreads();
}

// One workgroup of one wavefront per problem.  Problem p: in + p * nin, nin = (D + 1) D + (D + 1) + D + nDer doubles: the start cubes, their
// values, the posterior mean (theta | phi); hdr[2p] = leg (0 likelihood, 1 posterior), hdr[2p + 1] = a mean is given.  Out, 2 D + 2 nDer + 4
// doubles a problem: [cube | theta | phi | logL] of the best vertex, dXdtheta there (posterior leg), the likelihood at the mean (likelihood
// leg), the vertex's value, phi at the mean (likelihood leg); outi[2p], outi[2p + 1] = iterations that moved the simplex, likelihood calls of the search.
template <int DPL>
__global__ __launch_bounds__(64) void k_maximise(PcState S, const double *in, const int *hdr, long long max_iter, double *out, long long *outi)
{
    PC_DYN_LDS(smem);
    const int lane = threadIdx.x, D = S.D, n = D, nv = D + 1, p = blockIdx.x;
    double *ybuf = (double *)smem, *X = ybuf + D, *F = X + (size_t)nv * D, *M = F + nv;
    int *idx = (int *)(M + (size_t)D * D);
    const double *pin = in + (size_t)p * ((size_t)nv * D + nv + D + S.nDer);
    const int leg = __builtin_amdgcn_readfirstlane(hdr[2 * p]), has_mean = __builtin_amdgcn_readfirstlane(hdr[2 * p + 1]);
    LaneDims<DPL> ld; LaneTable<DPL> lt;
    pc_max_lanes<DPL>(S, lane, ld, lt, ybuf);
    for (int v = 0; v < nv; ++v) if (lane < D) X[v * D + lane] = pin[v * D + lane];
    for (int v = lane; v < nv; v += 64) { const double f0 = pin[nv * D + v]; F[v] = isfinite(f0) ? f0 : S.logzero; idx[v] = v; }
    const double dl = 1e-5;
    double det0 = -1.0;
    long long niter = 0, neval = 0;
    double xo[DPL], xw[DPL], xr[DPL], xt[DPL];
    for (long long iter = 0; iter < max_iter; ++iter) {
        pc_max_sort(F, idx, nv, lane);
        const int ib = __builtin_amdgcn_readfirstlane(idx[n]), iw = __builtin_amdgcn_readfirstlane(idx[0]), i2 = __builtin_amdgcn_readfirstlane(idx[1]);
        for (int c = 0; c < n; ++c) if (lane < D) M[c * n + lane] = X[idx[c] * D + lane] - X[ib * D + lane];      // edges from the best vertex
        const double det1 = fabs(pc_max_det(M, n, lane));
        if (det0 < 0.0) det0 = det1;
        const double fb = readlane_f64(F[ib], 0), fw = readlane_f64(F[iw], 0), f2 = readlane_f64(F[i2], 0);
        if (fb - fw < dl || !(det0 > 0.0) || readlane_f64(pow(det1 / det0, 1.0 / (double)n), 0) < dl) break;
        double s = 0.0;
        for (int k = 1; k <= n; ++k) s += ld.on[0] ? X[idx[k] * D + lane] : 0.0;      // centroid of all but the worst, summed in the order of idx
        xo[0] = ld.on[0] ? s / (double)n : 0.5;
        xw[0] = ld.on[0] ? X[iw * D + lane] : 0.5;
        xr[0] = xo[0] + (xo[0] - xw[0]);
        const double fr = pc_max_func<DPL>(S, ld, lt, xr, lane, ybuf, M, leg, neval);
        double fnew; bool shrink = false;
        if (fr <= fb && f2 < fr) { fnew = fr; xt[0] = xr[0]; }
        else if (fr > fb) {                                                // expansion
            xt[0] = xo[0] + 2.0 * (xr[0] - xo[0]);
            const double fe = pc_max_func<DPL>(S, ld, lt, xt, lane, ybuf, M, leg, neval);
            if (fe > fr) fnew = fe; else { fnew = fr; xt[0] = xr[0]; }
        } else {                                                           // contraction, else shrink towards the best
            xt[0] = xo[0] + 0.5 * (xw[0] - xo[0]);
            fnew = pc_max_func<DPL>(S, ld, lt, xt, lane, ybuf, M, leg, neval);
            shrink = !(fnew > fw);
        }
        if (!shrink) {
            if (lane < D) X[iw * D + lane] = xt[0];
            if (lane == 0) F[iw] = fnew;
        } else {
            for (int j = 0; j < n; ++j) {
                const int v = __builtin_amdgcn_readfirstlane(idx[j]);
                const double xb = ld.on[0] ? X[ib * D + lane] : 0.5, xv = ld.on[0] ? X[v * D + lane] : 0.5;
                xt[0] = xb + 0.5 * (xv - xb);
                if (lane < D) X[v * D + lane] = xt[0];
                const double fv = pc_max_func<DPL>(S, ld, lt, xt, lane, ybuf, M, leg, neval);
                if (lane == 0) F[v] = fv;
            }
        }
        ++niter;
    }
    pc_max_sort(F, idx, nv, lane);
    // calculate_point at the best vertex: theta, logL, and phi by the form's own path (as k_generate_live writes a row)
    const int ib = __builtin_amdgcn_readfirstlane(idx[n]);
    double *row = out + (size_t)p * (2 * D + 2 * S.nDer + 4);
    const int d0 = 2 * D, l0 = 2 * D + S.nDer;
    double xb[DPL], th[DPL];
    xb[0] = ld.on[0] ? X[ib * D + lane] : 0.5;
    th[0] = 0.0;
    double logL = S.logzero, dX = 0.0, lmean = 0.0;
    const double fbest = readlane_f64(F[ib], 0);
    const bool inside = pc_lanes(ld.on[0] && !(xb[0] >= 0.0 && xb[0] <= 1.0)) == 0ull;
    if (lane == 0) for (int e = 0; e < S.nDer; ++e) { row[d0 + e] = 0.0; row[l0 + 4 + e] = 0.0; }
    if (inside) {
        pc_max_theta<DPL>(S, ld, lt, xb, th, lane, ybuf);
        logL = pc_max_point<DPL>(S, ld, th, lane, ybuf, row + d0);
        if (leg == 1) dX = pc_max_dxdtheta<DPL>(S, ld, lt, xb, lane, ybuf, M);
    }
    if (leg == 0 && has_mean) {                                            // maximiser.F90:77-80: loglikelihood(mean theta) and the phi it gives there
        double tm[DPL];
        tm[0] = ld.on[0] ? pin[nv * D + nv + lane] : 0.0;
        lmean = pc_max_point<DPL>(S, ld, tm, lane, ybuf, row + l0 + 4);
    }
    if (lane < D) { row[lane] = xb[0]; row[D + lane] = th[0]; }
    if (lane == 0) {
        row[l0] = logL; row[l0 + 1] = dX; row[l0 + 2] = lmean; row[l0 + 3] = fbest;
        outi[2 * p] = niter; outi[2 * p + 1] = neval;
    }
}

// ------------------------------------------------------------------------------------------
// K1: one slice-sampling chain per wavefront
// ------------------------------------------------------------------------------------------
template <int DPL, int NROWS, int PT = 0>
struct ChainCtx {
    const PcState &S;
    const LaneDims<DPL> &ld;
    int lane;
    double *ybuf;
    int nlike;
    // Quadratic-form likelihoods (gaussian.f90, random_gaussian.f90) under a uniform prior: along a chord
    // theta(t) = theta0 + t s the exponent is  q(t) = qa + 2 qb t + qc t^2  with
    //   qa = y.M.y,  qb = s.M.y,  qc = s.M.s   (y = theta0 - mu; M = 1/sigma^2 or the inverse covariance),
    // all three reduced once per slice.  A trial is then a handful of scalar operations instead of a
    // wave reduction (or a D x D matrix-vector product) per likelihood call.  Every trial still counts as
    // one evaluation (calculate.f90:44).
    bool quad;
    double qa, qb, qc, qnorm;
#ifdef PCHIP_USER_TERMS
    double tsum[PC_NSUMS];   // the terms form: the sums of the last point eval_at evaluated -- the accepted point's, when a slice ends
    double *ybuf2;      // ... and LDS for a second theta (eval_pair: both bracket ends in one pass over the data)
#endif
};
// PT = 1: the same with the chain's prior table behind it (a non-linear prior has no closed form along the chord: quad stays false).
// A specialisation, so that the box's context -- and with it every kernel of a box run -- is what it was.
template <int DPL, int NROWS>
struct ChainCtx<DPL, NROWS, 1> {
    const PcState &S;
    const LaneDims<DPL> &ld;
    int lane;
    double *ybuf;
    int nlike;
    bool quad;
    double qa, qb, qc, qnorm;
    LaneTable<DPL> tb;
#ifdef PCHIP_USER_TERMS
    double tsum[PC_NSUMS];
    double *ybuf2;
#endif
};
// PT = 2 (a table with an adaptive block): the same members
template <int DPL, int NROWS>
struct ChainCtx<DPL, NROWS, 2> {
    const PcState &S;
    const LaneDims<DPL> &ld;
    int lane;
    double *ybuf;
    int nlike;
    bool quad;
    double qa, qb, qc, qnorm;
    LaneTable<DPL> tb;
#ifdef PCHIP_USER_TERMS
    double tsum[PC_NSUMS];
    double *ybuf2;
#endif
};

#ifdef PCHIP_USER_TERMS
// the two ends of a bracket (thA / thB: theta of the ends that are inside the cube, inA / inB wave-uniform): both in one pass over the
// data when both are inside, each counted as calculate.f90:44 counts it
template <int DPL, int NROWS, int PT>
__device__ __forceinline__ void like_pair_terms(ChainCtx<DPL, NROWS, PT> &C, const double (&thA)[DPL], const double (&thB)[DPL], bool inA, bool inB,
                                                double &lA, double &lB)
{
    const PcState &S = C.S;
    lA = S.logzero; lB = S.logzero;
    double sum[PC_NSUMS];
    if (inA && inB) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (C.ld.on[k]) { C.ybuf[C.lane + 64 * k] = thA[k]; C.ybuf2[C.lane + 64 * k] = thB[k]; }
        __syncthreads();
#ifdef PCHIP_USER_SHARED        // (both blocks behind one barrier)
        { const double *const two[2] = { C.ybuf, C.ybuf2 }; pc_shared_fill<2>(S, two, C.lane); }
#endif
        double sA[PC_NSUMS], sB[PC_NSUMS];
        pc_terms_sum2(S, C.ybuf, C.ybuf2, C.lane, sA, sB);
        double phi[PC_SRC_MAX_DERIVED];
        lA = pc_user_finish(sA, C.ybuf PC_SH_BLOCK(0), phi, S.D, S.nDer, S.src_data, (long)S.src_ndata);
        lB = pc_user_finish(sB, C.ybuf2 PC_SH_BLOCK(1), phi, S.D, S.nDer, S.src_data, (long)S.src_ndata);
        __syncthreads();
    } else if (inA) lA = like_eval_terms<DPL>(S, thA, C.ld, C.lane, C.ybuf, sum);
    else if (inB) lB = like_eval_terms<DPL>(S, thB, C.ld, C.lane, C.ybuf, sum);
    if (inA && lA > S.logzero) C.nlike++;
    if (inB && lB > S.logzero) C.nlike++;
}
#endif

// calculate_point (calculate.f90:6-50) at x0 + t*nh; leaves cube/theta of the trial in registers
template <int DPL, int NROWS, int KIND = -1, int PT = 0>
__device__ __forceinline__ double eval_at(ChainCtx<DPL, NROWS, PT> &C, const double (&x0)[DPL], const double (&nh)[DPL],
                                          double t, double (&cube)[DPL], double (&th)[DPL])
{
    bool outside = false;
    if (C.quad) {
        unsigned long long om = 0ull;               // the lanes outside the cube, as a mask: one scalar compare decides
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            cube[k] = x0[k] + t * nh[k];
            om |= (pc_lanes(cube[k] < 0.0) | pc_lanes(cube[k] > 1.0)) & pc_lanes(C.ld.on[k]);
            th[k] = C.ld.lo[k] + C.ld.span[k] * cube[k];
        }
        double lg = C.qnorm - (C.qa + t * (2.0 * C.qb + t * C.qc)) / 2.0;
        if (om != 0ull) {
#pragma unroll
            for (int k = 0; k < DPL; ++k) th[k] = 0.0;
            lg = C.S.logzero;                   // calculate.f90:36-38
        } else if (lg > C.S.logzero) C.nlike++;
        return lg;
    }
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        cube[k] = x0[k] + t * nh[k];
        if (C.ld.on[k]) outside |= (cube[k] < 0.0) | (cube[k] > 1.0);
    }
    if (__ballot(outside) != 0ull) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) th[k] = 0.0;
        return C.S.logzero;
    }
    if constexpr (PT != 0) PC_PRIOR_THETA(DPL, PT == 2, C.S, C.tb, cube, th, C.lane, C.ybuf);
    else {
#pragma unroll
    for (int k = 0; k < DPL; ++k) th[k] = C.ld.lo[k] + C.ld.span[k] * cube[k];
    }
#ifdef PCHIP_USER_TERMS     // (the sum stays with the chain: the derived parameters of the point a slice accepts are finish(sum))
    const double logL = (KIND < 0 && C.S.like.kind == PC_LIKE_SOURCE) ? like_eval_terms<DPL>(C.S, th, C.ld, C.lane, C.ybuf, C.tsum)
                                                                      : like_eval<DPL, NROWS, KIND>(C.S, th, C.ld, C.lane, C.ybuf);
#else
    const double logL = like_eval<DPL, NROWS, KIND>(C.S, th, C.ld, C.lane, C.ybuf);
#endif
    if (logL > C.S.logzero) C.nlike++;
    return logL;
}

// Two independent trial points at once (the two ends of the initial bracket): the per-point work is a
// dependent chain (FMA -> compare -> reduction), so the second evaluation rides in the shadow of the first.
// Straight-line code: both likelihoods are computed unconditionally and masked afterwards.
template <int DPL, int NROWS, int KIND = -1, int PT = 0>
__device__ __forceinline__ void eval_pair(ChainCtx<DPL, NROWS, PT> &C, const double (&x0)[DPL], const double (&nh)[DPL],
                                          double tA, double tB, double &lA, double &lB)
{
    const PcLike &L = C.S.like;
    const int kind = KIND >= 0 ? KIND : L.kind;
    if constexpr (PT != 0) {
        // a prior table: the outside-the-cube test first (calculate.f90:36-38; wave-uniform ballots), then the transform and the
        // likelihood of the points that are inside -- any kind through like_eval
        bool outA = false, outB = false;
        double cA[DPL], cB[DPL], thA[DPL], thB[DPL];
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            cA[k] = x0[k] + tA * nh[k]; cB[k] = x0[k] + tB * nh[k];
            if (C.ld.on[k]) { outA |= (cA[k] < 0.0) | (cA[k] > 1.0); outB |= (cB[k] < 0.0) | (cB[k] > 1.0); }
        }
        const bool oa = __ballot(outA) != 0ull, ob = __ballot(outB) != 0ull;
#ifdef PCHIP_USER_TERMS
        if (kind == PC_LIKE_SOURCE) {
            if (!oa) PC_PRIOR_THETA(DPL, PT == 2, C.S, C.tb, cA, thA, C.lane, C.ybuf);
            if (!ob) PC_PRIOR_THETA(DPL, PT == 2, C.S, C.tb, cB, thB, C.lane, C.ybuf);
            like_pair_terms<DPL, NROWS, PT>(C, thA, thB, !oa, !ob, lA, lB);
            return;
        }
#endif
        lA = C.S.logzero; lB = C.S.logzero;
        if (!oa) {
            PC_PRIOR_THETA(DPL, PT == 2, C.S, C.tb, cA, thA, C.lane, C.ybuf);
            lA = like_eval<DPL, NROWS, KIND>(C.S, thA, C.ld, C.lane, C.ybuf);
            if (lA > C.S.logzero) C.nlike++;
        }
        if (!ob) {
            PC_PRIOR_THETA(DPL, PT == 2, C.S, C.tb, cB, thB, C.lane, C.ybuf);
            lB = like_eval<DPL, NROWS, KIND>(C.S, thB, C.ld, C.lane, C.ybuf);
            if (lB > C.S.logzero) C.nlike++;
        }
        return;
    }
    if (C.quad) {
        unsigned long long oA = 0ull, oB = 0ull;     // the lanes outside the cube, as masks
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const double cA = x0[k] + tA * nh[k], cB = x0[k] + tB * nh[k];
            const unsigned long long on = pc_lanes(C.ld.on[k]);
            oA |= (pc_lanes(cA < 0.0) | pc_lanes(cA > 1.0)) & on; oB |= (pc_lanes(cB < 0.0) | pc_lanes(cB > 1.0)) & on;
        }
        lA = C.qnorm - (C.qa + tA * (2.0 * C.qb + tA * C.qc)) / 2.0;
        lB = C.qnorm - (C.qa + tB * (2.0 * C.qb + tB * C.qc)) / 2.0;
        // (calculate.f90:36-38; selects and a sum: no branch, no exec mask around one add)
        lA = oA != 0ull ? C.S.logzero : lA; lB = oB != 0ull ? C.S.logzero : lB;
        C.nlike += (int)(lA > C.S.logzero) + (int)(lB > C.S.logzero);
        return;
    }
    if (kind != PC_LIKE_RASTRIGIN && kind != PC_LIKE_TWIN_GAUSSIAN) {
        // any other functor (the quadratic built-ins when settings.ablate bit 0 takes their closed form away): the two points through
        // like_eval, one call behind the other in the source, their reductions side by side in the schedule
        // (until round 6 these kinds fell through to the twin-Gaussian sums below: an initial bracket judged by another likelihood never
        //  stepped out, and the "general functor" figures were those of a run with 3.3 evaluations a slice instead of 4.5)
        bool outA = false, outB = false;
        double thA[DPL], thB[DPL];
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const double cA = x0[k] + tA * nh[k], cB = x0[k] + tB * nh[k];
            if (C.ld.on[k]) { outA |= (cA < 0.0) | (cA > 1.0); outB |= (cB < 0.0) | (cB > 1.0); }
            thA[k] = C.ld.lo[k] + C.ld.span[k] * cA; thB[k] = C.ld.lo[k] + C.ld.span[k] * cB;
        }
        const bool oa = __ballot(outA) != 0ull, ob = __ballot(outB) != 0ull;
#ifdef PCHIP_USER_TERMS
        if (kind == PC_LIKE_SOURCE) { like_pair_terms<DPL, NROWS, PT>(C, thA, thB, !oa, !ob, lA, lB); return; }
#elif defined(PCHIP_USER_SOURCE)
        if (kind == PC_LIKE_SOURCE) {
            // the user's function only ever sees points inside the prior box (calculate.f90:36-38 tests the cube first); oa / ob are
            // wave-uniform ballots, so the barriers inside like_eval stay uniform
            lA = oa ? C.S.logzero : like_eval<DPL, NROWS, KIND>(C.S, thA, C.ld, C.lane, C.ybuf);
            lB = ob ? C.S.logzero : like_eval<DPL, NROWS, KIND>(C.S, thB, C.ld, C.lane, C.ybuf);
            if (!oa && lA > C.S.logzero) C.nlike++;
            if (!ob && lB > C.S.logzero) C.nlike++;
            return;
        }
#endif
        lA = like_eval<DPL, NROWS, KIND>(C.S, thA, C.ld, C.lane, C.ybuf);
        lB = like_eval<DPL, NROWS, KIND>(C.S, thB, C.ld, C.lane, C.ybuf);
        if (oa) lA = C.S.logzero; else if (lA > C.S.logzero) C.nlike++;     // calculate.f90:36-38
        if (ob) lB = C.S.logzero; else if (lB > C.S.logzero) C.nlike++;
        return;
    }
    bool outA = false, outB = false;
    double sA = 0.0, sB = 0.0, s2A = 0.0, s2B = 0.0;
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        const double cA = x0[k] + tA * nh[k], cB = x0[k] + tB * nh[k];
        if (C.ld.on[k]) { outA |= (cA < 0.0) | (cA > 1.0); outB |= (cB < 0.0) | (cB > 1.0); }
        const double thA = C.ld.lo[k] + C.ld.span[k] * cA, thB = C.ld.lo[k] + C.ld.span[k] * cB;
        if (C.ld.on[k]) {
            if (kind == PC_LIKE_RASTRIGIN) {
                sA += 8.515435146961291 + thA * thA - 10.0 * cos(PC_TWO_PI * thA);
                sB += 8.515435146961291 + thB * thB - 10.0 * cos(PC_TWO_PI * thB);
            } else {
                const int dim = C.lane + 64 * k;
                const double m1 = dim < 2 ? -0.5 : 0.0, m2 = dim < 2 ? 0.5 : 0.0;
                const double a1 = (thA - m1) * L.inv_sigma, a2 = (thA - m2) * L.inv_sigma;
                const double b1 = (thB - m1) * L.inv_sigma, b2 = (thB - m2) * L.inv_sigma;
                sA += a1 * a1; s2A += a2 * a2; sB += b1 * b1; s2B += b2 * b2;
            }
        }
    }
    const bool oa = __ballot(outA) != 0ull, ob = __ballot(outB) != 0ull;
    sA = wsum<DPL, NROWS>(sA); sB = wsum<DPL, NROWS>(sB);
    if (kind == PC_LIKE_RASTRIGIN) { lA = -sA; lB = -sB; }
    else {
        s2A = wsum<DPL, NROWS>(s2A); s2B = wsum<DPL, NROWS>(s2B);
        lA = pc_logaddexp(L.norm - sA / 2.0, L.norm - s2A / 2.0) - 0.6931471805599453;
        lB = pc_logaddexp(L.norm - sB / 2.0, L.norm - s2B / 2.0) - 0.6931471805599453;
    }
    if (oa) lA = C.S.logzero; else if (lA > C.S.logzero) C.nlike++;     // calculate.f90:36-38
    if (ob) lB = C.S.logzero; else if (lB > C.S.logzero) C.nlike++;
}

// SPECIAL = false is the production kernel.  SPECIAL = true adds the two rare modes, both decided at run time:
// more than one parameter grade (the evaluations of a slice are booked to the grade of its direction) and the
// sequential-stream test mode (every draw taken from ONE running stream in the reference's program order).
// WPB = chains (wavefronts) per workgroup.  One, except for the correlated Gaussian with its inverse covariance in LDS:
// an 80 KB matrix per chain left one wave per CU; WPB chains share one copy (every barrier below is executed the same
// number of times by every chain: per slice, never per likelihood evaluation).
// FW > 0 (production path for nDims <= 24, one grade): the kernel also does what the second half of k_nhats did -- seed
// choice (GenerateSeed) and whitening of the orthonormal directions with the seed cluster's Cholesky factor -- so that
// the directions never travel through HBM: a prologue whitens all of the chain's directions at once, lane = direction
// (the loops of k_nhats, bit for bit: row sums in ascending b, the norm on four partial sums), into LDS, from where the
// slices pick them up in deck order.  FW = unroll width >= nDims.
// PC_STEP_SPEC: the candidates of each side that the stepping out of a closed-form slice evaluates in straight-line code before its loop
// (pc_slice_body.inc; profiles/slice_stepping.json has the histogram it was chosen from).  0 = the loop alone, a developer build.
#ifndef PC_STEP_SPEC
#define PC_STEP_SPEC 1
#endif
constexpr int pc_step_spec = PC_STEP_SPEC;
// PC_SLICE_WAVES (build-time experiment): cap the registers so that this many waves share a SIMD
#ifdef PC_SLICE_WAVES
#define PC_SLICE_ATTR __attribute__((amdgpu_waves_per_eu(PC_SLICE_WAVES, PC_SLICE_WAVES)))
#else
#define PC_SLICE_ATTR
#endif
// PT = 1: the prior is a table (pc_table_theta) -- the general variants only (LEAN = 0, WPB = 1): no closed form along the chord;
// PT = 2: a table with an adaptive block (pc_table_theta<DPL, true>: the block structure is the point's), chosen by pc_table_pt
template <int DPL, int NROWS, bool SPECIAL, int WPB = 1, int FW = 0, int LEAN = 0, int PT = 0>
__global__ PC_SLICE_ATTR __launch_bounds__(64 * WPB * ((FW > 0 && (LEAN == 1 || LEAN == 3 || LEAN == 5) && WPB == 4) ? 2 : 1)) void k_slice(PcState S, unsigned batch, int phi_lds, int mat_lds)
{
#include "pc_slice_body.inc"
}

// several runs of a device in step (Cohort, pc_engine.hip): the same statements on each run's own state, blockIdx.y = run.  (Included, not
// called: handing the state to a function by reference moved fused multiply-adds in the one-run kernel -- -ffp-contract=fast works on
// whatever the optimiser has made of the code -- and the lane-per-chain kernel of pc_slice_t.hip is matched to that kernel's ISA.)
// PT as in k_slice (a prior table, a source prior): the general variants only, launched by pc_launch_slice_step; the six-argument names are the
// box's, as before
template <int DPL, int NROWS, bool SPECIAL, int WPB = 1, int FW = 0, int LEAN = 0, int PT = 0>
__global__ PC_SLICE_ATTR __launch_bounds__(64 * WPB) void k_slice_many(const PcManyRec *__restrict__ R, int phi_lds, int mat_lds)
{
    // (pointers left generic here: with them made global -- pc_many_state -- the compiler fused other multiply-adds than in the one-run
    //  kernel, the same statements, and a run in step was no longer bit for bit the run alone)
    const PcState S = R[blockIdx.y].S;
    const unsigned batch = (unsigned)R[blockIdx.y].ia[PC_REC_I_BATCH];
#include "pc_slice_body.inc"
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
#ifndef __HIPCC_RTC__         // (hiprtc, pc_rtc.hip: the kernels above, not the host code below)
#include "pc_launch.h"
#include <cstdio>
// The sampling kernels of a source likelihood (PC_LIKE_SOURCE), and of every kind under settings.ablate bit 15, come from a module that
// pc_rtc.hip compiles at run time from this very text: the launchers below choose the variant and its launch shape once, PC_LAUNCH sends
// it to the static kernel or, by its name, to the module's.
extern "C" int pc_rtc_wanted(const PcState *S) { return S->like.kind == PC_LIKE_SOURCE || (S->ablate & PC_ABL_RTC_BUILTINS) != 0; }
template <class... A> static int pc_rtc_go(const PcState *S, const char *expr, dim3 g, dim3 b, size_t sh, hipStream_t st, A... a)
{
    void *args[] = { (void *)&a... };
    return pc_rtc_launch(S, expr, g, b, sh, st, args);
}
#define PC_LAUNCH(K, G, B, SH, ST, ...) do { if (pc_rtc_wanted(S)) { if (pc_rtc_go(S, #K, G, B, SH, ST, __VA_ARGS__)) return 1; } \
                                             else hipLaunchKernelGGL(K, G, B, SH, ST, __VA_ARGS__); } while (0)
// the terms form of a source evaluates the two ends of a bracket in one pass over the data: LDS for the second theta behind the chain's block;
// a handle with several sums (pchip_source_create_sums) keeps the sums of every baby behind that, [nr][nsums], where the babies' theta rows
// are in LDS (phi_lds: pc_slice_phi_lds has counted this block in its decision); a quadratic form (pchip_source_create_quad) has its two
// residual blocks, 2 x nres doubles a chain (nres rounded up to even), in front of the chain's block, and a handle with shared values
// (pchip_source_create_shared) its two blocks of nshared doubles behind them: the form's front block, pc_front_lds, counted in that
// decision as well
static size_t pc_terms_lds(const PcState *S, const PcSourceForm &f, int phi_lds)
{
    if (f.nterms <= 0) return 0;
    return sizeof(double) * ((size_t)S->D + (phi_lds ? (size_t)S->nr * (size_t)f.nsums : 0)) + pc_front_lds(f);
}
// the form of a state's source, which every launcher of a kernel that evaluates the likelihood fetches once per call and hands to the
// helpers above and in pc_launch.h: one locked lookup in pc_rtc.hip's registry for a source state, none for any other (all zero).  A
// handle destroyed under a run in flight still answers (alive is not asked here): the cached kernel keeps its launch shape
static PcSourceForm pc_state_form(const PcState *S)
{
    PcSourceForm f{};
    if (S->like.kind == PC_LIKE_SOURCE) (void)pc_rtc_source_form(S->src_id, &f);
    return f;
}
// lane = coordinate: the coordinates a lane holds (template DPL) at nDims <= 64, 128, 256; 0 beyond (the launchers return 1)
static int pc_dpl(int D) { return D <= 64 ? 1 : (D <= 128 ? 2 : (D <= 256 ? 4 : 0)); }
extern "C" int pc_launch_generate_live(const PcState *S, int attempt0, int n, double *rows, double *rows_logL,
                                       hipStream_t st)
{
    const size_t sh = sizeof(double) * S->D + pc_front_lds(pc_state_form(S));
    const bool table = S->prior.kind >= 2;          // a prior table, or a source prior (kind 3: the same variants, from its handle's module)
    switch (pc_dpl(S->D) + (table ? 8 : 0)) {
    case 1: PC_LAUNCH((k_generate_live<1>), dim3(n), dim3(64), sh, st, *S, attempt0, rows, rows_logL); return 0;
    case 2: PC_LAUNCH((k_generate_live<2>), dim3(n), dim3(64), sh, st, *S, attempt0, rows, rows_logL); return 0;
    case 4: PC_LAUNCH((k_generate_live<4>), dim3(n), dim3(64), sh, st, *S, attempt0, rows, rows_logL); return 0;
    case 9: PC_LAUNCH((k_generate_live<1, 1>), dim3(n), dim3(64), sh, st, *S, attempt0, rows, rows_logL); return 0;
    case 10: PC_LAUNCH((k_generate_live<2, 1>), dim3(n), dim3(64), sh, st, *S, attempt0, rows, rows_logL); return 0;
    case 12: PC_LAUNCH((k_generate_live<4, 1>), dim3(n), dim3(64), sh, st, *S, attempt0, rows, rows_logL); return 0;
    }
    return 1;
}

extern "C" int pc_slice_fusable(const PcState *S)
{   // the slice kernel can do seeds + whitening itself: raw bases in HBM (split launch), one grade, nDims <= 24
    static const bool off = std::getenv("PC_SLICE_FUSED_OFF") != nullptr;
    return !off && S->D <= 24 && pc_nhats_splittable(S) && S->ngrade <= 1 && S->like.kind != PC_LIKE_CORR_GAUSSIAN && S->nr <= 1024;
}

// ------------------------------------------------------------------------------------------
// The launch of k_slice / k_slice_many: pc_slice_plan chooses the variant and the launch shape (every rule in one place),
// PC_SLICE_VARIANTS lists the variants that exist, pc_slice_launch sends a plan to its row.  A new variant: a rule in the
// plan and a row in the table.
// ------------------------------------------------------------------------------------------
// PT of a run behind a prior table or a source prior: 2 = the table has an adaptive block (its mask says so), 1 = any other
static int pc_table_pt(const PcState *S) { return S->prior.kind == 2 && ((unsigned)S->src_pad & PC_PT_ADAPTIVE) ? 2 : 1; }
struct PcSlicePlan {
    bool ok, many;                                // ok = false: no such launch (the launchers return 1);  many: k_slice_many, grid.y = run
    int dpl, nrows; bool special; int wpb, fw, lean, pt;      // the template arguments (see k_slice)
    dim3 grid, block; size_t lds;
    int phi_lds, mat_lds;                         // the kernels' run-time flags: theta rows of the babies / the inverse covariance in LDS
};

// The plan for a nursery of nchains chains: `fused` = seed choice and whitening inside the kernel (FW > 0, pc_slice_fusable), else the
// plain kernel behind k_nhats*;  R = 0: a run on its own (k_slice), R > 0: R runs of a device in step (k_slice_many: every run the same
// shape -- nDims, num_repeats, chains, likelihood kind).
static PcSlicePlan pc_slice_plan(const PcState *S, int nchains, int fused, int R)
{
    static const bool lean_off = std::getenv("PC_SLICE_LEAN_OFF") != nullptr, helper_off = std::getenv("PC_SLICE_HELPER_OFF") != nullptr,
                      wpb_off = std::getenv("PC_SLICE_WPB_OFF") != nullptr;
    PcSlicePlan p{};
    const int D = S->D, nr = S->nr;
    const bool table = S->prior.kind >= 2;                      // a prior table or a source prior (kind 3): every likelihood through like_eval, no matrix in LDS
    const bool special = S->ngrade > 1 || S->seq_mode;          // the two rare modes (pc_slice_fusable excludes both)
    const bool corr = S->like.kind == PC_LIKE_CORR_GAUSSIAN;
    if (D > 256 || (fused && !pc_slice_fusable(S))) return p;
    if (R && (table || (!fused && (corr || special || D > 64)))) return p;      // shapes only the one-run launchers take
    p.many = R > 0;
    p.dpl = pc_dpl(D);
    p.nrows = D <= 16 ? 1 : ((D <= 32 || fused) ? 2 : 4);
    p.special = special; p.wpb = 1; p.pt = table ? pc_table_pt(S) : 0;
    p.fw = !fused ? 0 : (D <= 8 ? 8 : (D <= 16 ? 16 : 24));
    p.grid = R ? dim3(nchains, R) : dim3(nchains); p.block = dim3(64);
    // a chain's LDS: ybuf + two int decks; theta of every baby (derived parameters at the end of the chain) when it fits
    const PcSourceForm f = pc_state_form(S);
    p.phi_lds = pc_slice_phi_lds(S, f);
    const size_t tb = sizeof(double) * (size_t)nr * (D + 1);
    size_t sh = sizeof(double) * ((size_t)D + nr) + 16 + (p.phi_lds ? tb : 0);
    if (fused) sh += sizeof(double) * ((size_t)p.fw * D + (size_t)nr * (D + 2));     // + L, directions, widths
    if (!R) sh += pc_terms_lds(S, f, p.phi_lds);                              // (a source in step: pc_launch_slice_step below, not this plan)
    if (fused && sh > 150 * 1024) return p;
    // the functor variants (LEAN = 3 Rastrigin, 4 twin Gaussian, 5 the Gaussian when settings.ablate bit 0 asks for it as a functor): one grade,
    // keyed draws, the box (a prior table: the general variants); runs in step take the Gaussian functor as the general kernel
    int leanf = 0;
    if (!lean_off && !special && !table)
        leanf = S->like.kind == PC_LIKE_RASTRIGIN ? 3 : (S->like.kind == PC_LIKE_TWIN_GAUSSIAN ? 4 : ((S->like.kind == PC_LIKE_GAUSSIAN && (S->ablate & PC_ABL_FUNCTOR) && !R) ? 5 : 0));
    if (fused) {
        // LEAN = 1: the Gaussian in closed form along the chord, its deck in registers (one-run launches)
        const bool lean = !R && !lean_off && !table && S->like.kind == PC_LIKE_GAUSSIAN && !(S->ablate & PC_ABL_FUNCTOR) && p.phi_lds && nr <= 64 && !special;
        p.lean = leanf ? leanf : (lean ? 1 : 0);
        // four chains a workgroup with their four helper wavefronts (pc_slice_body.inc): the lean variants whose deck lives in registers (1, 3, 5),
        // nurseries of a multiple of four chains; settings.ablate bit 13 / PC_SLICE_HELPER_OFF: one wavefront a workgroup as before (the same numbers)
        const size_t pw4 = ((size_t)D + nr + (p.phi_lds ? (size_t)nr * (D + 1) : 0) + (size_t)p.fw * D + (size_t)nr * (D + 2) + (size_t)((nr + 3) / 4) * 128 + (size_t)nr + 1) & ~(size_t)1;
        const size_t sh4 = 4 * sizeof(double) * pw4 + 16;
        if (!R && (p.lean == 1 || p.lean == 3 || p.lean == 5) && !helper_off && !(S->ablate & PC_ABL_NO_HELPER) && nr <= 64 && (nchains & 3) == 0 && sh4 <= 150 * 1024) {
            p.wpb = 4; p.grid = dim3(nchains / 4); p.block = dim3(512); sh = sh4;
        }
    } else {
        // the inverse covariance of the correlated Gaussian in LDS when it fits (and its products are not in HBM: nhat_Ms)
        const size_t mb = sizeof(double) * (size_t)D * D;
        p.mat_lds = (!table && corr && S->nhat_Ms == nullptr && sh + mb <= 150 * 1024) ? 1 : 0;
        if (p.mat_lds && D > 64 && D <= 128 && nchains % 4 == 0 && !special && !wpb_off && 4 * sh + mb <= 150 * 1024) {
            // four chains per workgroup around one LDS copy of the inverse covariance (65 <= nDims <= 128)
            p.wpb = 4; p.grid = dim3(nchains / 4); p.block = dim3(256); sh = 4 * sh + mb;
        } else {
            if (p.mat_lds) sh += mb;
            // BASELINE configs[4]'s shape: the kernel without its other variants (LEAN = 2)
            if (!lean_off && !table && corr && S->nhat_Ms != nullptr && !(S->ablate & PC_ABL_FUNCTOR) && S->nDer == 0 && nr > 64 && D > 64 && D <= 128 && !special) p.lean = 2;
            else if (D <= 64) p.lean = leanf;
        }
    }
    p.lds = sh; p.ok = true;
    return p;
}

// Tables with an adaptive block (PT = 2, pc_table_pt): the twin of every PT = 1 row of the tables below -- of PC_SLICE_VARIANTS for k_slice, of
// PC_SLICE_STEP_VARIANTS for k_slice_many -- in tables of their own behind them: those two list what every other run takes, as before.
#define PC_SLICE_ADAPT_VARIANTS(X) \
    X(1, 1, false, 1, 0, 0, 2) X(1, 1, true, 1, 0, 0, 2) X(1, 2, false, 1, 0, 0, 2) X(1, 2, true, 1, 0, 0, 2) X(1, 4, false, 1, 0, 0, 2) X(1, 4, true, 1, 0, 0, 2) X(2, 4, false, 1, 0, 0, 2) X(2, 4, true, 1, 0, 0, 2) X(4, 4, false, 1, 0, 0, 2) X(4, 4, true, 1, 0, 0, 2) X(1, 1, false, 1, 8, 0, 2) X(1, 1, false, 1, 16, 0, 2) X(1, 2, false, 1, 24, 0, 2)
#define PC_SLICE_STEP_ADAPT_VARIANTS(X) \
    X(1, 1, false, 1, 0, 0, 2) X(1, 2, false, 1, 0, 0, 2) X(1, 4, false, 1, 0, 0, 2) X(1, 1, false, 1, 8, 0, 2) X(1, 1, false, 1, 16, 0, 2) X(1, 2, false, 1, 24, 0, 2)

// the instantiations of k_slice: DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT  (a prior table: the rows k_slice<DPL, NROWS, GR, 1, 0, 0, 1> and, fused,
// k_slice<1, NROWS, false, 1, FW, 0, 1>; their twins PT = 2: PC_SLICE_ADAPT_VARIANTS above)
#define PC_SLICE_VARIANTS(X) \
    /* behind k_nhats*: nDims <= 16, 32, 64, 128, 256; general (box / table prior, without / with the rare modes) and functors */ \
    X(1, 1, false, 1, 0, 0, 0) X(1, 1, true, 1, 0, 0, 0) X(1, 1, false, 1, 0, 0, 1) X(1, 1, true, 1, 0, 0, 1) X(1, 1, false, 1, 0, 3, 0) X(1, 1, false, 1, 0, 4, 0) X(1, 1, false, 1, 0, 5, 0) \
    X(1, 2, false, 1, 0, 0, 0) X(1, 2, true, 1, 0, 0, 0) X(1, 2, false, 1, 0, 0, 1) X(1, 2, true, 1, 0, 0, 1) X(1, 2, false, 1, 0, 3, 0) X(1, 2, false, 1, 0, 4, 0) X(1, 2, false, 1, 0, 5, 0) \
    X(1, 4, false, 1, 0, 0, 0) X(1, 4, true, 1, 0, 0, 0) X(1, 4, false, 1, 0, 0, 1) X(1, 4, true, 1, 0, 0, 1) X(1, 4, false, 1, 0, 3, 0) X(1, 4, false, 1, 0, 4, 0) X(1, 4, false, 1, 0, 5, 0) \
    X(2, 4, false, 1, 0, 0, 0) X(2, 4, true, 1, 0, 0, 0) X(2, 4, false, 1, 0, 0, 1) X(2, 4, true, 1, 0, 0, 1) \
    X(4, 4, false, 1, 0, 0, 0) X(4, 4, true, 1, 0, 0, 0) X(4, 4, false, 1, 0, 0, 1) X(4, 4, true, 1, 0, 0, 1) \
    /* the correlated Gaussian, 65 <= nDims <= 128: four chains around one matrix in LDS; its products from HBM (LEAN = 2) */ \
    X(2, 4, false, 4, 0, 0, 0) X(2, 4, false, 1, 0, 2, 0) \
    /* fused, nDims <= 8, 16, 24: general (box / table), then LEAN = 1, 3, 4, 5 with one chain and with four chains + helpers a workgroup */ \
    /* (WPB = 4 with LEAN = 4 is compiled and never chosen: the twin Gaussian's functor has no helper wavefront) */ \
    X(1, 1, false, 1, 8, 0, 0) X(1, 1, false, 1, 8, 0, 1) X(1, 1, false, 1, 8, 1, 0) X(1, 1, false, 4, 8, 1, 0) X(1, 1, false, 1, 8, 3, 0) X(1, 1, false, 4, 8, 3, 0) X(1, 1, false, 1, 8, 4, 0) X(1, 1, false, 4, 8, 4, 0) X(1, 1, false, 1, 8, 5, 0) X(1, 1, false, 4, 8, 5, 0) \
    X(1, 1, false, 1, 16, 0, 0) X(1, 1, false, 1, 16, 0, 1) X(1, 1, false, 1, 16, 1, 0) X(1, 1, false, 4, 16, 1, 0) X(1, 1, false, 1, 16, 3, 0) X(1, 1, false, 4, 16, 3, 0) X(1, 1, false, 1, 16, 4, 0) X(1, 1, false, 4, 16, 4, 0) X(1, 1, false, 1, 16, 5, 0) X(1, 1, false, 4, 16, 5, 0) \
    X(1, 2, false, 1, 24, 0, 0) X(1, 2, false, 1, 24, 0, 1) X(1, 2, false, 1, 24, 1, 0) X(1, 2, false, 4, 24, 1, 0) X(1, 2, false, 1, 24, 3, 0) X(1, 2, false, 4, 24, 3, 0) X(1, 2, false, 1, 24, 4, 0) X(1, 2, false, 4, 24, 4, 0) X(1, 2, false, 1, 24, 5, 0) X(1, 2, false, 4, 24, 5, 0)
// ... and of k_slice_many (no PT: runs in step take the box only): DPL, NROWS, SPECIAL, WPB, FW, LEAN
#define PC_SLICE_MANY_VARIANTS(X) \
    X(1, 1, false, 1, 0, 0) X(1, 1, false, 1, 0, 3) X(1, 1, false, 1, 0, 4) X(1, 2, false, 1, 0, 0) X(1, 2, false, 1, 0, 3) X(1, 2, false, 1, 0, 4) X(1, 4, false, 1, 0, 0) X(1, 4, false, 1, 0, 3) X(1, 4, false, 1, 0, 4) \
    X(1, 1, false, 1, 8, 0) X(1, 1, false, 1, 8, 3) X(1, 1, false, 1, 8, 4) X(1, 1, false, 1, 16, 0) X(1, 1, false, 1, 16, 3) X(1, 1, false, 1, 16, 4) X(1, 2, false, 1, 24, 0) X(1, 2, false, 1, 24, 3) X(1, 2, false, 1, 24, 4)

// 0: launched; 1: no such launch, the run-time module failed (pc_rtc_error), or the plan names a variant that is not in the table (a programming error)
static int pc_slice_launch(const PcState *S, const PcSlicePlan &p, const PcManyRec *dR, unsigned batch, hipStream_t st)
{
    if (!p.ok) return 1;
#define PC_ROW(DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT) \
    if (!p.many && p.dpl == DPL && p.nrows == NROWS && p.special == SPECIAL && p.wpb == WPB && p.fw == FW && p.lean == LEAN && p.pt == PT) { \
        if (p.lds > 48 * 1024) pc_need_dyn_lds((const void *)k_slice<DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT>, p.lds); \
        PC_LAUNCH((k_slice<DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT>), p.grid, p.block, p.lds, st, *S, batch, p.phi_lds, p.mat_lds); \
        return 0; }
    PC_SLICE_VARIANTS(PC_ROW)
    PC_SLICE_ADAPT_VARIANTS(PC_ROW)
#undef PC_ROW
#define PC_ROW(DPL, NROWS, SPECIAL, WPB, FW, LEAN) \
    if (p.many && p.dpl == DPL && p.nrows == NROWS && p.special == SPECIAL && p.wpb == WPB && p.fw == FW && p.lean == LEAN && p.pt == 0) { \
        if (p.lds > 48 * 1024) pc_need_dyn_lds((const void *)k_slice_many<DPL, NROWS, SPECIAL, WPB, FW, LEAN>, p.lds); \
        PC_LAUNCH((k_slice_many<DPL, NROWS, SPECIAL, WPB, FW, LEAN>), p.grid, p.block, p.lds, st, dR, p.phi_lds, p.mat_lds); \
        return 0; }
    PC_SLICE_MANY_VARIANTS(PC_ROW)
#undef PC_ROW
    char msg[160];
    std::snprintf(msg, sizeof msg, "pc_slice_launch: no %s<%d, %d, %d, %d, %d, %d, %d> in the variant table", p.many ? "k_slice_many" : "k_slice",
                  p.dpl, p.nrows, (int)p.special, p.wpb, p.fw, p.lean, p.pt);
    pc_abi_set_last_error(msg);
    return 1;
}

extern "C" int pc_launch_slice(const PcState *S, unsigned batch, int nchains, hipStream_t st) { return pc_slice_launch(S, pc_slice_plan(S, nchains, 0, 0), nullptr, batch, st); }
extern "C" int pc_launch_slice_fused(const PcState *S, unsigned batch, int nchains, hipStream_t st) { return pc_slice_launch(S, pc_slice_plan(S, nchains, 1, 0), nullptr, batch, st); }
// Several runs of a device in step: the sampling kernel of any device likelihood launched once for all of them (grid.y = run).
// 1: a shape only the one-run launchers take.
extern "C" int pc_launch_slice_many(const PcState *S, const PcManyRec *dR, int R, int nchains, int fused, hipStream_t st) { return pc_slice_launch(S, pc_slice_plan(S, nchains, fused, R), dR, 0u, st); }

// ------------------------------------------------------------------------------------------
// Runs in step whose problem is the user's own: a source likelihood (plain or terms form) and / or a device prior (a table, a source
// prior).  pc_slice_plan and its tables above stay what they were (the box, the built-ins); the rules here are the plan's for R > 0 without
// its refusal of a table, with the terms form's LDS, and never a functor variant: the general kernel, PT = 0 (a source under the box)
// or 1 (2: a table with an adaptive block).  DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT as above; the PT = 0 rows are the instantiations of PC_SLICE_MANY_VARIANTS' LEAN = 0 rows.
// ------------------------------------------------------------------------------------------
#define PC_SLICE_STEP_VARIANTS(X) \
    X(1, 1, false, 1, 0, 0, 0) X(1, 2, false, 1, 0, 0, 0) X(1, 4, false, 1, 0, 0, 0) X(1, 1, false, 1, 8, 0, 0) X(1, 1, false, 1, 16, 0, 0) X(1, 2, false, 1, 24, 0, 0) \
    X(1, 1, false, 1, 0, 0, 1) X(1, 2, false, 1, 0, 0, 1) X(1, 4, false, 1, 0, 0, 1) X(1, 1, false, 1, 8, 0, 1) X(1, 1, false, 1, 16, 0, 1) X(1, 2, false, 1, 24, 0, 1)

// the plan for R runs in step, nchains chains each; ok = false: a shape without a shared launch (each run then launches its own k_slice, which
// takes any shape: nDims 65 ... 256, grades, the sequential stream, the correlated Gaussian)
static PcSlicePlan pc_slice_step_plan(const PcState *S, int nchains, int fused, int R)
{
    PcSlicePlan p{};
    const int D = S->D, nr = S->nr;
    if (R < 1 || nchains < 1 || D < 1) return p;
    if (S->ngrade > 1 || S->seq_mode || S->like.kind == PC_LIKE_CORR_GAUSSIAN) return p;
    if (fused ? !pc_slice_fusable(S) : D > 64) return p;
    p.many = true;
    p.dpl = 1;
    p.nrows = D <= 16 ? 1 : ((D <= 32 || fused) ? 2 : 4);
    p.special = false; p.wpb = 1; p.lean = 0; p.pt = S->prior.kind >= 2 ? pc_table_pt(S) : 0;
    p.fw = !fused ? 0 : (D <= 8 ? 8 : (D <= 16 ? 16 : 24));
    p.grid = dim3(nchains, R); p.block = dim3(64);
    // a chain's LDS as pc_slice_plan lays it out, and the second theta of the terms form (and the babies' sums) behind it
    const PcSourceForm f = pc_state_form(S);
    p.phi_lds = pc_slice_phi_lds(S, f);
    size_t sh = sizeof(double) * ((size_t)D + nr) + 16 + (p.phi_lds ? sizeof(double) * (size_t)nr * (D + 1) : 0);
    if (fused) sh += sizeof(double) * ((size_t)p.fw * D + (size_t)nr * (D + 2));
    sh += pc_terms_lds(S, f, p.phi_lds);
    if (fused && sh > 150 * 1024) return p;
    p.lds = sh; p.ok = true;
    return p;
}

// 0: launched once for the R runs; 1: no shared launch for this shape, or the run-time module failed (pc_rtc_error)
extern "C" int pc_launch_slice_step(const PcState *S, const PcManyRec *dR, int R, int nchains, int fused, hipStream_t st)
{
    const PcSlicePlan p = pc_slice_step_plan(S, nchains, fused, R);
    if (!p.ok) return 1;
#define PC_ROW(DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT) \
    if (p.dpl == DPL && p.nrows == NROWS && p.special == SPECIAL && p.wpb == WPB && p.fw == FW && p.lean == LEAN && p.pt == PT) { \
        if (p.lds > 48 * 1024) pc_need_dyn_lds((const void *)k_slice_many<DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT>, p.lds); \
        PC_LAUNCH((k_slice_many<DPL, NROWS, SPECIAL, WPB, FW, LEAN, PT>), p.grid, p.block, p.lds, st, dR, p.phi_lds, p.mat_lds); \
        return 0; }
    PC_SLICE_STEP_VARIANTS(PC_ROW)
    PC_SLICE_STEP_ADAPT_VARIANTS(PC_ROW)
#undef PC_ROW
    char msg[160];
    std::snprintf(msg, sizeof msg, "pc_launch_slice_step: no k_slice_many<%d, %d, %d, %d, %d, %d, %d> in the variant table", p.dpl, p.nrows, (int)p.special, p.wpb, p.fw, p.lean, p.pt);
    pc_abi_set_last_error(msg);
    return 1;
}

// pchip_prior_transform: the device transform of the table in S->prior at n points (device pointers)
extern "C" int pc_launch_prior_transform(const PcState *S, int n, const double *cubes, double *thetas, hipStream_t st)
{
    if ((S->prior.kind != 2 && S->prior.kind != 1) || n < 1) return 1;
    const size_t sh = sizeof(double) * S->D;
    switch (pc_dpl(S->D)) {
    case 1: hipLaunchKernelGGL((k_prior_transform<1>), dim3(n), dim3(64), sh, st, *S, cubes, thetas); return 0;
    case 2: hipLaunchKernelGGL((k_prior_transform<2>), dim3(n), dim3(64), sh, st, *S, cubes, thetas); return 0;
    case 4: hipLaunchKernelGGL((k_prior_transform<4>), dim3(n), dim3(64), sh, st, *S, cubes, thetas); return 0;
    }
    return 1;
}

// pchip_source_eval: a source likelihood at n points (device pointers), by the handle's run-time module -- there is no static kernel
extern "C" int pc_launch_source_eval(const PcState *S, int n, const double *thetas, double *logL, double *phi, hipStream_t st)
{
    const int dpl = pc_dpl(S->D);
    if (S->like.kind != PC_LIKE_SOURCE || n < 1 || !dpl) return 1;
    const char *name = dpl == 1 ? "k_source_eval<1>" : (dpl == 2 ? "k_source_eval<2>" : "k_source_eval<4>");
    return pc_rtc_go(S, name, dim3(n), dim3(64), sizeof(double) * S->D + pc_front_lds(pc_state_form(S)), st, *S, thetas, logL, phi);
}

// pchip_source_prior_eval: the prior of a source handle at n points (device pointers) -- k_prior_transform of the handle's run-time module
extern "C" int pc_launch_source_prior_eval(const PcState *S, int n, const double *cubes, double *thetas, hipStream_t st)
{
    const int dpl = pc_dpl(S->D);
    if (S->like.kind != PC_LIKE_SOURCE || S->prior.kind != 3 || n < 1 || !dpl) return 1;
    const char *name = dpl == 1 ? "k_prior_transform<1>" : (dpl == 2 ? "k_prior_transform<2>" : "k_prior_transform<4>");
    return pc_rtc_go(S, name, dim3(n), dim3(64), sizeof(double) * S->D, st, *S, cubes, thetas);
}

// the device maximiser (pchip_maximise_device): nDims <= 64, any device likelihood under prior kinds 1, 2, 3; the LDS block is held against the
// device's limit per workgroup (the message in polychord_hip_last_error)
static int pc_max_lds_fits(const char *who, size_t sh)
{
    int dev = 0, lim = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || sh > (size_t)lim) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "%s: %zu bytes of LDS, the device has %d", who, sh, lim);
        pc_abi_set_last_error(msg);
        (void)hipGetLastError();
        return 0;
    }
    return 1;
}
extern "C" int pc_launch_max_rank(const PcState *S, int n, const double *rows, double *val, hipStream_t st)
{
    if (S->D < 1 || S->D > 64 || n < 1) return 1;
    const size_t sh = sizeof(double) * ((size_t)S->D + (size_t)S->D * S->D);
    if (!pc_max_lds_fits("k_max_rank", sh)) return 1;
    if (sh > 48 * 1024 && !pc_rtc_wanted(S)) pc_need_dyn_lds((const void *)k_max_rank<1>, sh);
    PC_LAUNCH((k_max_rank<1>), dim3(n), dim3(64), sh, st, *S, rows, val);
    return 0;
}
extern "C" int pc_launch_maximise(const PcState *S, int nprob, const double *in, const int *hdr, long long max_iter, double *out, long long *outi, hipStream_t st)
{
    if (S->D < 1 || S->D > 64 || nprob < 1) return 1;
    const size_t sh = sizeof(double) * PC_MAX_LDS_DOUBLES(S->D) + pc_front_lds(pc_state_form(S));
    if (!pc_max_lds_fits("k_maximise", sh)) return 1;
    if (sh > 48 * 1024 && !pc_rtc_wanted(S)) pc_need_dyn_lds((const void *)k_maximise<1>, sh);
    PC_LAUNCH((k_maximise<1>), dim3(nprob), dim3(64), sh, st, *S, in, hdr, max_iter, out, outi);
    return 0;
}
#endif  // __HIPCC_RTC__
