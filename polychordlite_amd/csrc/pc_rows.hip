// pc_rows.hip -- the row kernels: they execute the PLAN a contraction kernel emitted (k_consume of pc_contract.hip and its kin), in parallel
// over the whole chip: dead rows, phantoms, new live rows.
//
//   k_apply_dead_ph, k_apply_live   slot mode: the dead row and the phantoms of every consumed chain, then the new occupants of the slots
//   k_apply_pool                    pool mode: both in ONE launch, no row copied to become a phantom
//   k_apply_pool_flag               ... with the workgroups of the one-cluster update's flag pass (pc_upd_flag.h) in front of its own
//   k_install_live                  the initial live set: rows -> slots, labels, contour
#include "pc_state.h"
#include "pc_launch.h"
#include "pc_block.h"
#include "pc_upd_flag.h"
#include <algorithm>
#include <cstdlib>

// ------------------------------------------------------------------------------------------
// apply the plan: dead rows + phantoms (reads live[] before k_apply_live overwrites slots)
// one wave per consumed chain
// ------------------------------------------------------------------------------------------
// four waves per consumed chain: wave 0 also moves the dead row; the phantoms of a mask word are shared out among the
// waves by runs of bits (a wave's rows go to consecutive rows behind those of the waves before it)
#define PC_APPLY_WAVES 4
__device__ __forceinline__ void apply_dead_ph_body(const PcState &S, unsigned batch)
{
    const PcCtl *ctl = S.ctl;
    const int w = ctl->seg_lo + blockIdx.x;
    if (w > ctl->seg_hi) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nT = S.nT, nr = S.nr;
    const int di = S.plan[w].dead_idx;
    if (di >= 0 && wv == 0) {
        const int src = S.plan[w].dead_src;
        const double *row = (src >= 0) ? S.live + (size_t)src * nT
                                       : S.babies + ((size_t)(-src - 1) * nr + (nr - 1)) * nT;
        double *dst = S.dead + (size_t)di * nT;
        for (int e = lane; e < nT; e += 64) dst[e] = row[e];
        if (lane == 0) {
            S.dead_logw[di] = S.plan[w].logw; S.dead_postX[di] = S.plan[w].postX + log(S.plan[w].postXs); S.dead_postZ[di] = S.plan[w].postZ;
            S.dead_cuid[di] = S.plan[w].dead_cuid;
            S.dead_entry[di] = (src >= 0) ? S.live_entry[src] : S.plan[-src - 1].contour;
        }
    }
    int base = S.plan[w].ph_base;
    const unsigned cuid = S.plan[w].ph_cuid;
    if (S.plan[w].ph_count == -2) {
        // a region of nr rows for this chain (parallel contraction): baby i is a phantom if it lies above the contour
        // the chain was consumed at and then occupies row base + i; the rest of the region is marked with PC_CUID_NONE
        const double Lg = S.plan[w].contour;
        for (int m = 0; m < (nr + 63) / 64; ++m) {
            const int i = m * 64 + lane;
            const double bl = (i < nr) ? S.baby_logL[(size_t)w * nr + i] : -PC_HUGE;
            const bool sel = (i < nr - 1) && bl > Lg;
            const unsigned long long mask = __ballot(sel);
            if (wv == 0 && i < nr) {
                S.ph_logL[base + i] = bl; S.ph_cuid[base + i] = sel ? cuid : PC_CUID_NONE;
                S.ph_uid[base + i] = ((unsigned long long)batch << 32) | (unsigned)(w * nr + i);
            }
            // wave k copies the rows of bits [16k, 16k + 16), eight in flight
            unsigned long long mine = mask & (0xFFFFull << (16 * wv));
            const double *src0 = S.babies + ((size_t)w * nr + m * 64) * nT;
            double *dst0 = S.phantom + (size_t)(base + m * 64) * nT;
            while (mine) {
                int idx[8], cnt = 0;
#pragma unroll
                for (int u = 0; u < 8; ++u) { idx[u] = 0; if (mine) { idx[u] = __ffsll((long long)mine) - 1; mine &= mine - 1; cnt = u + 1; } }
                for (int e = lane; e < nT; e += 64) {
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) if (u < cnt) v[u] = src0[(size_t)idx[u] * nT + e];
#pragma unroll
                    for (int u = 0; u < 8; ++u) if (u < cnt) dst0[(size_t)idx[u] * nT + e] = v[u];
                }
            }
        }
        return;
    }
    for (int m = 0; m < (nr + 62) / 64; ++m) {
        const unsigned long long mask = S.plan[w].ph_mask[m];
        // side arrays: lane b of wave 0 owns baby m*64+b, its row offset is the number of selected babies before it
        if (wv == 0 && ((mask >> lane) & 1ull)) {
            const int i = m * 64 + lane, dsti = base + __popcll(mask & ((1ull << lane) - 1ull));
            S.ph_logL[dsti] = S.baby_logL[(size_t)w * nr + i]; S.ph_cuid[dsti] = cuid;
            S.ph_uid[dsti] = ((unsigned long long)batch << 32) | (unsigned)(w * nr + i);
        }
        // wave k takes bits [16k, 16k + 16)
        const unsigned long long mine = mask & (0xFFFFull << (16 * wv));
        const int before = __popcll(mask & ((1ull << (16 * wv)) - 1ull));
        wave_copy_masked(S.babies + ((size_t)w * nr + m * 64) * nT, mine, S.phantom + (size_t)(base + before) * nT, nT, lane);
        base += __popcll(mask);
    }
}
__global__ __launch_bounds__(64 * PC_APPLY_WAVES) void k_apply_dead_ph(PcState S, unsigned batch) { apply_dead_ph_body(S, batch); }
__global__ __launch_bounds__(64 * PC_APPLY_WAVES) void k_apply_dead_ph_many(const PcManyRec *__restrict__ R) { apply_dead_ph_body(pc_many_state(R, blockIdx.y), (unsigned)R[blockIdx.y].ia[PC_REC_I_BATCH]); }

// pool mode: both of the above in ONE launch (a kernel boundary on the main stream costs 6 us, 79 times per run at the metric
// configuration).  No row is copied to become a phantom, so a chain's workgroup only writes the side arrays of its region and,
// if the point that died at its step was a newcomer of this launch, that baby's row; the rows of snapshot points that died
// are moved out by the workgroup of their SLOT (k_consume_par left the killer's chain in slot_dead) just before the slot's
// new occupant moves in -- the one place where the order of the two copies matters.
// (four wavefronts a workgroup, a chain or a slot each: with one wavefront a workgroup the launch was as long as the dispatcher
//  took to hand 3000 workgroups out -- 192 k of them for sixty-four runs in step, 122 us)
// IDS = false (k_apply_pool_flag): the ids of the chains' rows are written by the flag workgroups of the same launch (pc_upd_flag.h).
template <bool IDS>
__device__ __forceinline__ void apply_pool_body(const PcState &S, unsigned batch, int nchains, int wg)
{
    const PcCtl *ctl = S.ctl;
    const int lane = threadIdx.x & 63, nT = S.nT, nr = S.nr;
    const int item = wg * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);      // (wg: the workgroup's number among the row kernel's)
    if (item >= nchains + S.Ncap) return;
    if (item < nchains) {
        const int w = ctl->seg_lo + item;
        if (w > ctl->seg_hi) return;
        const int di = S.plan[w].dead_idx, src = S.plan[w].dead_src;
        if (di >= 0 && src < 0) {
            const double *row = S.babies + ((size_t)(-src - 1) * nr + (nr - 1)) * nT;
            double *dst = S.dead + (size_t)di * nT;
            for (int e = lane; e < nT; e += 64) dst[e] = row[e];
            if (lane == 0) {
                S.dead_logw[di] = S.plan[w].logw; S.dead_postX[di] = S.plan[w].postX + log(S.plan[w].postXs); S.dead_postZ[di] = S.plan[w].postZ;
                S.dead_cuid[di] = S.plan[w].dead_cuid; S.dead_entry[di] = S.plan[-src - 1].contour;
            }
        }
        if (!IDS) return;
        const int base = S.plan[w].ph_base;
        const unsigned cuid = S.plan[w].ph_cuid;
        const double Lg = S.plan[w].contour;
        for (int i = lane; i < nr; i += 64) {
            const double bl = S.baby_logL[(size_t)w * nr + i];
            S.ph_logL[base + i] = bl; S.ph_cuid[base + i] = ((i < nr - 1) && bl > Lg) ? cuid : PC_CUID_NONE;
            S.ph_uid[base + i] = ((unsigned long long)batch << 32) | (unsigned)(w * nr + i);
        }
        return;
    }
    const int slot = item - nchains;
    const int src = S.slot_src[slot], killer = S.slot_dead[slot];
    if (src < 0 && killer < 0) return;
    double *lrow = S.live + (size_t)slot * nT;
    if (killer >= 0) {
        const int di = S.plan[killer].dead_idx;
        double *dst = S.dead + (size_t)di * nT;
        for (int e = lane; e < nT; e += 64) dst[e] = lrow[e];
        if (lane == 0) {
            S.dead_logw[di] = S.plan[killer].logw; S.dead_postX[di] = S.plan[killer].postX + log(S.plan[killer].postXs); S.dead_postZ[di] = S.plan[killer].postZ;
            S.dead_cuid[di] = S.plan[killer].dead_cuid; S.dead_entry[di] = S.live_entry[slot];
        }
    }
    if (src >= 0) {
        const double *row = S.babies + ((size_t)src * nr + (nr - 1)) * nT;
        double v[4];                                    // (nTotal <= 256 elements a lane: the loads before the stores)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (lane + 64 * q < nT) ? row[lane + 64 * q] : 0.0;
        for (int e = lane + 256; e < nT; e += 64) lrow[e] = row[e];
#pragma unroll
        for (int q = 0; q < 4; ++q) if (lane + 64 * q < nT) lrow[lane + 64 * q] = v[q];
    }
    // (a lane's copies are in program order, and the slot's records below are its wavefront's alone: no barrier)
    if (lane == 0) { S.slot_src[slot] = -1; S.slot_dead[slot] = -1; if (src >= 0) S.live_entry[slot] = S.plan[src].contour; }
}
__global__ __launch_bounds__(256) void k_apply_pool(PcState S, unsigned batch, int nchains) { apply_pool_body<true>(S, batch, nchains, (int)blockIdx.x); }
__global__ __launch_bounds__(256) void k_apply_pool_many(const PcManyRec *R, int nchains) { apply_pool_body<true>(pc_many_state(R, blockIdx.y), (unsigned)R[blockIdx.y].ia[PC_REC_I_BATCH], nchains, (int)blockIdx.x); }
// the row kernel and the update's flag pass in one launch: workgroups [0, nb_flag) take four blocks of 256 phantom rows each, like k_upd_flag's
// (in front: theirs is the longer chain of dependent loads when an update is pending), the ones behind them are k_apply_pool's.  Nobody waits
// for anybody: what the flag pass needs of this round's rows it forms itself.
__global__ __launch_bounds__(256) void k_apply_pool_flag(PcState S, unsigned batch, int nchains, int nb_flag, int nph, unsigned char *keep, int *blk, int nblk)
{
    if ((int)blockIdx.x >= nb_flag) { apply_pool_body<false>(S, batch, nchains, (int)blockIdx.x - nb_flag); return; }
    upd_flag_body<true>(S, nph, keep, blk, 1, nblk, (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), batch);
}


// new live rows: every slot now owned by a chain's last baby
__device__ __forceinline__ void apply_live_body(const PcState &S)
{
    const int slot = blockIdx.x, lane = threadIdx.x, nT = S.nT, nr = S.nr;
    const int src = S.slot_src[slot];
    if (src < 0) return;
    const double *row = S.babies + ((size_t)src * nr + (nr - 1)) * nT;
    double *dst = S.live + (size_t)slot * nT;
    for (int e = lane; e < nT; e += 64) dst[e] = row[e];
    __syncthreads();
    if (lane == 0) { S.slot_src[slot] = -1; S.live_entry[slot] = S.plan[src].contour; }
}
__global__ __launch_bounds__(64) void k_apply_live(PcState S) { apply_live_body(S); }
__global__ __launch_bounds__(64) void k_apply_live_many(const PcManyRec *__restrict__ R) { apply_live_body(pc_many_state(R, blockIdx.y)); }

// ------------------------------------------------------------------------------------------
// install the initial live set: rows -> slots, labels, contour (generate.F90:291-320)
// single workgroup; also trims nprior > nlive through k_consume(final)-like deaths on the host side
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_install_live(PcState S, const double *rows, int n)
{
    const int tid = threadIdx.x;
    __shared__ vk_t red[4];
    for (int s = tid; s < S.Ncap; s += 256) {
        if (s < n) {                                       // (the rows themselves: one device-to-device copy in front of this launch)
            S.live_logL[s] = rows[(size_t)s * S.nT + S.l0]; S.live_cluster[s] = 0; S.live_pos[s] = s; S.live_entry[s] = S.logzero;
            S.cl_list[s] = s;
        } else { S.live_logL[s] = PC_HUGE; S.live_cluster[s] = -1; S.live_pos[s] = 0; S.live_entry[s] = S.logzero; }
        S.slot_src[s] = -1;
    }
    __syncthreads();
    vk_t best{PC_HUGE, 0x7fffffff};
    double mx = -PC_HUGE;
    for (int s = tid; s < n; s += 256) { best = vk_min(best, vk_t{S.live_logL[s], s}); mx = fmax(mx, S.live_logL[s]); }
    best = block_argmin<256>(best, red);
    __shared__ double smx[4];
    mx = wave_max(mx);
    if ((tid & 63) == 0) smx[tid >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3]));
    double sum = 0.0;
    for (int s = tid; s < n; s += 256) sum += exp(S.live_logL[s] - mx);
    sum = wave_sum<4>(sum);
    __syncthreads();
    if ((tid & 63) == 0) smx[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        S.cl_n[0] = n; S.logLp[0] = best.v; S.imin_slot[0] = best.k;
        S.lse_ref[0] = mx; S.lse_sum[0] = (smx[0] + smx[1]) + (smx[2] + smx[3]);
    }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
extern "C" void pc_launch_apply(const PcState *S, unsigned batch, int nchains, hipStream_t st)
{
    if (S->pool) { hipLaunchKernelGGL(k_apply_pool, dim3((nchains + S->Ncap + 3) / 4), dim3(256), 0, st, *S, batch, nchains); return; }
    hipLaunchKernelGGL(k_apply_dead_ph, dim3(nchains), dim3(64 * PC_APPLY_WAVES), 0, st, *S, batch);
    hipLaunchKernelGGL(k_apply_live, dim3(S->Ncap), dim3(64), 0, st, *S);
}

extern "C" void pc_launch_apply_flag(const PcState *S, unsigned batch, int nchains, int nph, unsigned char *keep, int *blk, hipStream_t st)
{
    const int nb_apply = (nchains + S->Ncap + 3) / 4, nblk = (nph + UPD_ROWS - 1) / UPD_ROWS, nb_flag = (nblk + 3) / 4;
    hipLaunchKernelGGL(k_apply_pool_flag, dim3(nb_flag + nb_apply), dim3(256), 0, st, *S, batch, nchains, nb_flag, nph, keep, blk, nblk);
}

// PC_APPLY_WAVES, a developer switch (wavefronts a workgroup of k_apply_pool_many, 1 ... 4), read once per process
static int apply_pool_many_waves()
{
    static const int w = [] { const char *e = std::getenv("PC_APPLY_WAVES"); return e ? std::max(1, std::min(4, std::atoi(e))) : 4; }();
    return w;
}
extern "C" int pc_launch_apply_many(const PcState *S, const PcManyRec *dR, int R, unsigned batch, int nchains, hipStream_t st)
{
    if (!S->pool) {      // (the runs of a launch share the layout: Cohort::flush groups them by it)
        hipLaunchKernelGGL(k_apply_dead_ph_many, dim3(nchains, R), dim3(64 * PC_APPLY_WAVES), 0, st, dR);
        hipLaunchKernelGGL(k_apply_live_many, dim3(S->Ncap, R), dim3(64), 0, st, dR);
        return 0;
    }
    const int wpg = apply_pool_many_waves();
    hipLaunchKernelGGL(k_apply_pool_many, dim3((nchains + S->Ncap + wpg - 1) / wpg, R), dim3(64 * wpg), 0, st, dR, nchains);      // (the nursery's number: each run's own, PcManyRec::ia[PC_REC_I_BATCH])
    return 0;
}

extern "C" void pc_launch_install_live(const PcState *S, const double *rows, int n, hipStream_t st)
{
    if (n > 0) (void)hipMemcpyAsync(S->live, rows, sizeof(double) * (size_t)n * S->nT, hipMemcpyDeviceToDevice, st);
    hipLaunchKernelGGL(k_install_live, dim3(1), dim3(256), 0, st, *S, rows, n);
}
