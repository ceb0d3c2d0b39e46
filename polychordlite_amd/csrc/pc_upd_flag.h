// pc_upd_flag.h -- the first stage of the one-cluster update: which phantom rows survive, survivors per block of 256 rows.  Device code, shared
// by the update's own launch (pc_update.hip: k_upd_flag, k_upd_flag_many, k_upd_flag_scan) and by the row kernel of a run on its own in pool mode
// (pc_rows.hip: k_apply_pool_flag), whose launch carries the workgroups of this pass in front of its own.
#pragma once
#include "pc_state.h"

#define UPD_ROWS 256
#define UPD_NT 256

// def (here and below): the update is made AFTER the launch of the parallel contraction that passed its trigger, for the
// state at the mark the launch recorded (PcCtl::upd_*): the threshold of the clean is the logL of the death at the mark;
// the moments leave out what came after it -- phantoms of later chains, live points accepted later -- and take in the
// points that were alive then and have died since (their rows are in the dead array)
// (a wavefront takes one block of the counts -- 256 rows, four consecutive rows per lane: 32-byte, 16-byte and 4-byte accesses in
//  place of 8, 4 and 1 -- and a workgroup four of them; the survivors of a block are counted by ballots, no LDS)
// a value another workgroup of the SAME launch reads behind a ticket (upd_ticket_last): stored write-through at agent scope, so that the
// ticket needs no release fence (a release writes back the whole L2 of the XCD -- with the sampling kernel's rows still dirty there)
template <typename T> __device__ __forceinline__ void upd_store_wt(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// sb: the wavefront's block of rows.
// REGION (pool mode, deferred, in the row kernel's launch): the rows of the chains that the contraction in front of this launch consumed --
// [pool_base + seg_lo nr, pool_base + (seg_hi + 1) nr) -- have no ids in memory yet: the chain items of the SAME launch used to write them, and
// nothing orders one workgroup behind another.  So this pass forms their ph_logL / ph_cuid / ph_uid itself, from baby_logL and the chain's plan
// record exactly as the chain item did, flags them from the values in registers and writes ids and flags in one go; the chain items write no ids
// then.  The ids are due in every round, the flags only when the contraction left an update pending (PcCtl::upd_pending, which the host cannot know
// when it enqueues the launch): a wavefront whose block has no such row returns at once when none is.
template <bool REGION>
__device__ __forceinline__ void upd_flag_body(const PcState &S, int nph, unsigned char *keep, int *blk_count, int def, int nblk, int sb, unsigned batch = 0u)
{
    const int lane = threadIdx.x & 63;
    if (sb >= nblk) return;
    const int nr = S.nr;
    const int j0 = sb * UPD_ROWS + 4 * lane;
    bool pending = true;
    int r_lo = 0, r_hi = 0;                            // REGION: the rows whose ids this pass forms
    if (REGION) {
        const PcCtl *ctl = S.ctl;
        pending = ctl->upd_pending != 0;
        r_lo = S.pool_base + ctl->seg_lo * nr; r_hi = S.pool_base + (ctl->seg_hi + 1) * nr;
        if (!pending && !(sb * UPD_ROWS < r_hi && sb * UPD_ROWS + UPD_ROWS > r_lo)) return;      // (uniform in the wavefront)
    }
    const unsigned uid0 = S.cl_uid[0];
    const double thr = def ? S.ctl->upd_thr : S.death_thr[0];
    const bool pool = S.pool;
    // pool mode: a dropped phantom is dropped where it lies; the rows that count in the moments (the survivors that were
    // phantoms at the mark -- rows of chains consumed later stay, but do not count) are listed by k_upd_index
    const int tmark = (pool && def) ? S.ctl->upd_tmark : 0x7fffffff, nph0u = (pool && def) ? S.ctl->upd_nph0 : 0x7fffffff;
    const int T = (pool && def) ? S.ctl->upd_T : 0;
    const bool full = j0 + 3 < nph;
    const bool mixed = REGION && j0 < r_hi && j0 + 3 >= r_lo;      // some of the lane's four rows get their ids here
    unsigned cu[4] = {PC_CUID_NONE, PC_CUID_NONE, PC_CUID_NONE, PC_CUID_NONE};
    double ll[4] = {0.0, 0.0, 0.0, 0.0};
    if (mixed) {
        // (the region is one interval: behind the lane's first row in it -- one division -- the baby and the chain are stepped)
        int w = 0, i = 0; bool in = false; double Lg = 0.0; unsigned pc = PC_CUID_NONE;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u;
            if (j >= nph) continue;
            if (j >= r_lo && j < r_hi) {
                if (!in) { const int q = j - S.pool_base; w = q / nr; i = q - w * nr; in = true; Lg = S.plan[w].contour; pc = S.plan[w].ph_cuid; }
                else if (++i == nr) { i = 0; ++w; Lg = S.plan[w].contour; pc = S.plan[w].ph_cuid; }
                const double bl = S.baby_logL[j - S.pool_base];      // (baby i of chain w is row w nr + i of the nursery)
                ll[u] = bl; cu[u] = ((i < nr - 1) && bl > Lg) ? pc : PC_CUID_NONE;
            } else { cu[u] = S.ph_cuid[j]; ll[u] = S.ph_logL[j]; }
        }
    } else if (full) {
        const uint4 c = *(const uint4 *)(S.ph_cuid + j0);
        const double2 a = *(const double2 *)(S.ph_logL + j0), b2 = *(const double2 *)(S.ph_logL + j0 + 2);
        cu[0] = c.x; cu[1] = c.y; cu[2] = c.z; cu[3] = c.w; ll[0] = a.x; ll[1] = a.y; ll[2] = b2.x; ll[3] = b2.y;
    } else {
        for (int u = 0; u < 4; ++u) if (j0 + u < nph) { cu[u] = S.ph_cuid[j0 + u]; ll[u] = S.ph_logL[j0 + u]; }
    }
    unsigned kb = 0; bool wr = false; int cnt = 0;
    if (pending) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u;
            bool k = false, km = false;
            if (j < nph) {
                k = (cu[u] == uid0) && !(ll[u] < thr);
                if (pool) {
                    if (!k && cu[u] == uid0) { cu[u] = PC_CUID_NONE; wr = true; }
                    km = k && (j < nph0u || T - 1 - (j - nph0u) / nr < tmark);
                }
                kb |= (unsigned)((k ? 1 : 0) | (km ? 2 : 0)) << (8 * u);
            }
            cnt += __popcll(__ballot(pool ? km : k));
        }
        if (full) *(unsigned *)(keep + j0) = kb;
        else for (int u = 0; u < 4; ++u) if (j0 + u < nph) keep[j0 + u] = (unsigned char)((kb >> (8 * u)) & 0xFFu);
    }
    if (mixed && full && j0 >= r_lo && j0 + 3 < r_hi) {      // all four rows: the accesses of the rows that are in memory
        const unsigned long long u0 = ((unsigned long long)batch << 32) | (unsigned)(j0 - S.pool_base);
        *(double2 *)(S.ph_logL + j0) = make_double2(ll[0], ll[1]); *(double2 *)(S.ph_logL + j0 + 2) = make_double2(ll[2], ll[3]);
        *(uint4 *)(S.ph_cuid + j0) = make_uint4(cu[0], cu[1], cu[2], cu[3]);
        *(ulonglong2 *)(S.ph_uid + j0) = make_ulonglong2(u0, u0 + 1); *(ulonglong2 *)(S.ph_uid + j0 + 2) = make_ulonglong2(u0 + 2, u0 + 3);
    } else if (mixed) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u;
            if (j >= nph) continue;
            if (j >= r_lo && j < r_hi) {
                S.ph_logL[j] = ll[u]; S.ph_cuid[j] = cu[u];
                S.ph_uid[j] = ((unsigned long long)batch << 32) | (unsigned)(j - S.pool_base);
            } else if (wr) S.ph_cuid[j] = cu[u];
        }
    } else if (wr) {
        if (full) *(uint4 *)(S.ph_cuid + j0) = make_uint4(cu[0], cu[1], cu[2], cu[3]);
        else for (int u = 0; u < 4; ++u) if (j0 + u < nph) S.ph_cuid[j0 + u] = cu[u];
    }
    if (pending && lane == 0) upd_store_wt(blk_count + sb, cnt);        // (write-through: the chain's last arriver reads it in this launch)
}
