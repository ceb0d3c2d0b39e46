// pc_consume_clp_body.inc -- the body of k_consume_clp (pc_clus.hip), included by the one-run kernel and by k_consume_clp_many (several runs
// in step, blockIdx.y = run): the same statements on `S`.  Not a header: no include guard.
//
// The contraction of a clustered run with its DECISIONS made in parallel (round 6).  k_consume_cl (pc_consume_cl_body.inc) walks the nursery with one
// wavefront, ~700 instructions a chain, issue bound: 40-50 % of a clustered BASELINE run.  What a chain's fate depends on is little:
//   (i)  the contour at its turn, Lg_t = the (k_t + 1)-th smallest of S u A_t (S the sorted snapshot of the live set, A_t the candidates -- last
//        babies -- accepted before step t, k_t their number): with a static number of live points every acceptance is a death, the dead are the
//        k_t smallest, and `c_t > Lg_t` is a statement about RANKS,  #{e in S : e < c_t}  >  Q(t, rank_t),  where
//        Q(t, r) = #{s < t accepted : rank_s >= r}  (pc_par.hip's rule for one cluster);
//   (ii) identify_cluster (run_time_info.f90:913-949) of its last baby: the first of <= 8 listed candidates that is alive at step t.  A point x of
//        the snapshot (sorted index i_x, r_x candidates below it) is alive at step t iff it is not among the k_t smallest:  i_x >= Q(t, r_x);  the
//        last baby of an earlier chain v iff it was accepted and  #{e in S : e <= c_v} >= Q(t, rank_v).
// So the acceptance vector a is the fixed point of a map whose every entry asks a few dominance counts Q(t, r).  Wave 0 resolves it 64 steps at a
// time, lane = step: Q splits into the settled part (a bitmap of accepted ranks with word-level suffix counts: two LDS reads) and the part inside
// the chunk (popcount of the guessed acceptance ballot under a 64-bit mask of the chunk's ranks >= r, built once per chunk and only for the
// candidates whose fate can change inside the chunk -- the <= 64 lowest living points); the in-chunk dependencies settle in 2-7 rounds (each round
// fixes at least the first unsettled step).  Everything else a consumed chain leaves behind follows from a WITHOUT a serial walk, all threads:
// the j-th death is the j-th entry of the merge of S and the accepted candidates, the slot a newcomer inherits by pointer jumping over "who died
// for whom", a cluster's live count at a death by counting the earlier deaths and additions of that cluster, its volume by the product of their
// ratios in order (the same multiplications in the same order as the serial kernel), the phantom masks from a table (cluster, step of birth, step
// of death) per candidate, the counters by prefix sums, the step that ends the launch -- update trigger (nested_sampling.F90:321), a cluster's
// death (:339), max_ndead, nfail, the window of the linear-space evidence -- as a minimum over the steps.  Steps behind that end are forgotten.
// update_evidence, the live evidence / more_samples_needed and the list bookkeeping stay what they were: waves 1, 2, 3 of k_consume_cl, following
// the records of the consumed chains (they now find them all in place).
// A baby whose candidate list holds no living entry needs the full search over the live set AS IT IS at its step (a handful of chains per run):
// the pass ends in front of such a step, the state is written back, and the next pass finds the chain at its step 0, where the staged state is
// the live set it must be searched in.
// Same decisions as k_consume_cl and k_consume: tests/test_gpu_parity.py test_clustered_contraction_kernels_agree (settings.ablate bit 10 = the
// serial one-wave kernel, bit 5 = the general kernel), the clustered oracle cases, both epoch rules.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Ncap = S.Ncap, maxc = S.maxc, nr = S.nr, nT = S.nT, D = S.D;
    const int NS = (Ncap + 63) & ~63, nw = (nr + 63) / 64;
    const ClpLayout Y = clp_layout(Ncap, S.B, nr);
    ClSlot *sS = (ClSlot *)(smem + Y.slot); double *sL = (double *)(smem + Y.sL);
    ClSL *sSort = (ClSL *)(smem + Y.sorted); unsigned short *sSlotOf = (unsigned short *)(smem + Y.sortSlot); ClSL *sCand = (ClSL *)(smem + Y.cand);
    ClChain *sCh = (ClChain *)(smem + Y.chain); ClHead *sHead = (ClHead *)(smem + Y.head); ClOwn *sOwn = (ClOwn *)(smem + Y.own);
    double *slogn = (double *)(smem + Y.logn), *srcp = (double *)(smem + Y.rcp), *fg = (double *)(smem + Y.fg);
    unsigned long long *masks = (unsigned long long *)(smem + Y.masks), *kmin = (unsigned long long *)(smem + Y.kmin);
    int *sCS = (int *)(smem + Y.sCS), *lst = (int *)(smem + Y.lst), *lstOff = (int *)(smem + Y.lstOff);
    unsigned *tag = (unsigned *)(smem + Y.tag);
    ClEvt *sEvt = (ClEvt *)(smem + Y.evt);
    unsigned short *idxOf = (unsigned short *)(smem + Y.idxOf), *rxS = (unsigned short *)(smem + Y.rxS), *belowS = (unsigned short *)(smem + Y.below),
                   *belowE = belowS + S.B, *kAcc = (unsigned short *)(smem + Y.kacc), *sU = (unsigned short *)(smem + Y.U), *stepOf = (unsigned short *)(smem + Y.stepOf),
                   // (the deaths' tables take the place of the interleaving tables, which the order of deaths -- B1 -- is the last to read)
                   *link = rxS, *slotD = belowS, *cdca = belowS + (S.B + 2);
    unsigned long long *accW = (unsigned long long *)(smem + Y.accw);       // [16] accepted candidates by rank
    int *sufW = (int *)(accW + 16);                                        // [17] accepted candidates in the words >= l
    unsigned short *ctot = (unsigned short *)(smem + Y.ctot);              // [groups of 64 deaths][CL_MAXC] deaths | additions << 8 of a cluster inside a group
    int *clN0 = (int *)(smem + Y.clN), *clAdd = clN0 + CL_MAXC, *clLastJ = clAdd + CL_MAXC;      // a cluster's live count at launch, its net change, its last death
    unsigned *clUid = (unsigned *)(clLastJ + CL_MAXC);
    int *clDead = (int *)(clUid + CL_MAXC);                                // the step at which a cluster lost its last point (CLP_ALIVE: it has not)
    double *clX0 = (double *)(smem + Y.clX), *clThr = clX0 + CL_MAXC;
    double *ratD = (double *)masks;                                        // [B] a death's volume ratio n / (n + 1): in the masks' LDS until the masks are made
    double *Fbuf = fg, *Gbuf = fg + CL_MAXC;
    __shared__ int out_i[16];
    __shared__ double out_d[8];
    __shared__ double ref_d[8];        // launch-wide references: Lhi, lxm0
    __shared__ int lp_prog, lp_done, lp_stop, lp_lists;      // chains >= lp_prog are decided; the decisions are done; first chain that must not be consumed (-2: none); chains >= lp_lists are in the lists
    __shared__ int pa_Tp, pa_K, pa_end, pa_hard, pa_jupd;       // steps decided, acceptances among them, the code of the step that ends the pass, first step with a baby no list resolves, the death that triggers the update
    __shared__ double pa_sum0, pa_sum_end;
    __shared__ long long pa_scan[3 * (CLP_NT / 64)];
    __shared__ long long out_l[4];

    PcCtl *ctl = S.ctl;
    const long long t_start = clock64();
    int seg_hi_launch = -1;
    int redo_limit = CL_NO_LIMIT;                     // the chain that ends a pass made again (the precision criterion: see CL_MEET)
    int hard_cap = 0x7fffffff;                        // ... or the step such a pass ends in front of (a phantom candidate that asks for the full search)
    // the full search of identify_cluster (run_time_info.f90:913-949) for ONE baby over the live set as the LDS holds it, by one wavefront
    auto full_search = [&](int w, int bi) -> int {
        const double *x = S.babies + ((size_t)w * nr + bi) * nT;
        vk_t best{PC_HUGE, 0x7fffffff};
        for (int s = lane; s < Ncap; s += 64) {
            const int rc = sS[s].c, ro = sS[s].o;
            if (rc < 0) continue;
            const double *y = (ro >= 0) ? S.babies + ((size_t)ro * nr + (nr - 1)) * nT : S.live + (size_t)s * nT;
            double d2 = 0.0;
            for (int d = 0; d < D; ++d) { const double t = x[d] - y[d]; d2 += t * t; }
            best = vk_min(best, vk_t{d2, rc * Ncap + sS[s].p});
        }
        best = wave_argmin(best);
        return (best.k == 0x7fffffff) ? -1 : best.k / Ncap;
    };
    for (int pass = 0;; ++pass) {
    const long long t_pass = clock64();
    long long t_meet = 0;
    const int T = ctl->i_nursery;                     // chains in the nursery at launch: w = T-1 ... 0, step t = T-1-w
    int nc = ctl->ncluster;
    const int epoch0 = ctl->admin_epoch;
    // ------------------------------------------------------------------ stage (all waves)
    {
        constexpr int SB = 4;
        for (int s0 = tid; s0 < Ncap; s0 += CLP_NT * SB) {
            double l[SB]; int c[SB], pp[SB], o[SB], sr[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int s = s0 + u * CLP_NT; const bool in = s < Ncap; const int si = in ? s : 0;
                                           l[u] = S.live_logL[si]; c[u] = S.live_cluster[si]; pp[u] = S.live_pos[si]; o[u] = S.nn_slot_owner[si]; sr[u] = S.slot_src[si]; }
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int s = s0 + u * CLP_NT; if (s < Ncap) { sL[s] = l[u]; sS[s] = ClSlot{c[u], pp[u], o[u], sr[u]}; idxOf[s] = 0xFFFFu; } }
        }
        for (int i0 = tid; i0 <= NS; i0 += CLP_NT * SB) {
            unsigned long long k[SB]; int sl[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int i = i0 + u * CLP_NT; const bool in = i < NS; k[u] = in ? S.sort_key[i] : 0ull; sl[u] = in ? S.sort_slot[i] : -1; }
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int i = i0 + u * CLP_NT; if (i <= NS) { sSort[i] = ClSL{i < NS ? key2d(k[u]) : PC_HUGE, 0.0}; sSlotOf[i] = (unsigned short)(sl[u] < 0 ? 0xFFFF : sl[u]); } }
        }
        for (int c0 = tid; c0 < S.B; c0 += CLP_NT * SB) {
            int v[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int c = c0 + u * CLP_NT; v[u] = c < S.B ? S.nn_chain_slot[c] : 0; }
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int c = c0 + u * CLP_NT; if (c < S.B) sCS[c] = v[u]; }
        }
        for (int w0 = tid; w0 < T; w0 += CLP_NT * SB) {
            double bl[SB]; int nl[SB], ep[SB], cc[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int w = w0 + u * CLP_NT; const int wi = w < T ? w : 0;
                                           bl[u] = S.baby_logL[(size_t)wi * nr + nr - 1]; nl[u] = S.ch_nlike[wi]; ep[u] = S.ch_epoch[wi]; cc[u] = S.ch_cluster[wi]; }
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int w = w0 + u * CLP_NT; if (w < T) sCh[w] = ClChain{bl[u], nl[u], ep[u], cc[u], 0}; }
        }
        for (int k0 = tid; k0 < Ncap + 4; k0 += CLP_NT * SB) {
            double v[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int k = k0 + u * CLP_NT; v[u] = k < Ncap + 4 ? S.logn[k] : 0.0; }
#pragma unroll
            for (int u = 0; u < SB; ++u) { const int k = k0 + u * CLP_NT; if (k < Ncap + 4) { slogn[k] = v[u]; srcp[k] = k > 0 ? 1.0 / (double)k : 0.0; } }
        }
        if (tid < CL_MAXC) { const bool in = tid < nc; clN0[tid] = in ? S.cl_n[tid] : 0; clAdd[tid] = 0; clLastJ[tid] = -1; clUid[tid] = in ? S.cl_uid[tid] : 0u; clThr[tid] = in ? S.death_thr[tid] : -PC_HUGE; clDead[tid] = CLP_ALIVE; }
        if (tid < 16) accW[tid] = 0ull;
        if (tid < 17) sufW[tid] = 0;
    }
    __syncthreads();
    // the sorted index of every slot's occupant (0xFFFF: a free slot)
    for (int i = tid; i < NS; i += CLP_NT) { const unsigned sl = sSlotOf[i]; if (sl != 0xFFFFu && sSort[i].L < PC_HUGE) idxOf[sl] = (unsigned short)i; }
    // per-cluster lists with room for the chains that may join: a cluster's region = its points + the nursery's chains seeded in it
    { int *kcnt = (int *)sHead;                                         // (128 counters in the plan records' LDS, which nothing has written yet)
      for (int c = tid; c < CL_MAXC; c += CLP_NT) kcnt[c] = 0;
      __syncthreads();
      for (int w = tid; w < T; w += CLP_NT) { const int ca = sCh[w].ca; if (ca >= 0 && ca < CL_MAXC) atomicAdd(&kcnt[ca], 1); }
      __syncthreads();
      if (tid < nc) kmin[tid] = (unsigned long long)kcnt[tid]; }
    if (tid == CLP_NT - 1) {
        // the window of this launch: its k-th death lies below the k-th smallest point of the snapshot
        int nlv = 0;
        for (int c = 0; c < nc; ++c) nlv += clN0[c];
        const int kth = (T < nlv ? T : nlv) - 1;
        const double L0 = sSort[0].L, Lk = sSort[kth > 0 ? kth : 0].L;
        ref_d[0] = fmin(Lk, L0 + CL_WINDOW);
        double m = -PC_HUGE;
        for (int c = 0; c < nc; ++c) m = fmax(m, S.logXp[c]);
        ref_d[1] = m;
        out_i[11] = nlv;
    }
    __syncthreads();
    const double Lhi = ref_d[0], lxm0 = ref_d[1];
    const int nlv = out_i[11];
    if (tid == 0) { int o = 0; for (int c = 0; c < nc; ++c) { lstOff[c] = o; o += clN0[c] + (int)kmin[c]; } lstOff[nc] = o; }
    if (tid < nc) {
        // own accumulators of a cluster: each about the larger of its value now and the largest term this launch can add
        ClOwn o;
        const double zp0 = S.logZp[tid], zpx0 = S.logZpXp[tid], zp20 = S.logZp2[tid];
        o.rzp = fmax(zp0, lxm0 + Lhi); o.zp = exp(zp0 - o.rzp); o.kzp = exp(lxm0 + Lhi - o.rzp);
        o.rzpx = fmax(zpx0, 2.0 * lxm0 + Lhi); o.zpx = exp(zpx0 - o.rzpx); o.kzpx = exp(2.0 * lxm0 + Lhi - o.rzpx);
        o.rzp2 = fmax(zp20, fmax(o.rzpx + Lhi, 2.0 * lxm0 + 2.0 * Lhi)); o.zp2 = exp(zp20 - o.rzp2);
        o.kp2a = exp(o.rzpx + Lhi - o.rzp2); o.kp2b = exp(2.0 * lxm0 + 2.0 * Lhi - o.rzp2);
        o.touched = 0; o.pad = 0;
        sOwn[tid] = o;
        clX0[tid] = exp(S.logXp[tid] - lxm0);
    }
    __syncthreads();
    for (int s = tid; s < Ncap; s += CLP_NT) if (sS[s].c >= 0) lst[lstOff[sS[s].c] + sS[s].p] = s;
    // ranks of the candidates (last babies) among themselves: (logL, chain) ascending, by integer key (a strict total order whatever the values)
    {
        int np2 = 2;
        while (np2 < T) np2 <<= 1;
        unsigned long long *kk = (unsigned long long *)sHead;          // [np2]  (sizeof(ClHead) * B >= 12 * 2 B bytes)
        int *kw = (int *)(kk + np2);                                    // [np2]
        for (int i = tid; i < np2; i += CLP_NT) { kk[i] = i < T ? d2key(sCh[i].last) : KEY_HUGE; kw[i] = i < T ? i : 0x7fffffff; }
        __syncthreads();
        for (int k = 2; k <= np2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < np2; i += CLP_NT) {
                    const int l = i ^ j;
                    if (l > i) {
                        const bool up = (i & k) == 0;
                        const unsigned long long a = kk[i], b = kk[l]; const int wa = kw[i], wb = kw[l];
                        const bool gt = (a > b) || (a == b && wa > wb);
                        if (gt == up) { kk[i] = b; kk[l] = a; kw[i] = wb; kw[l] = wa; }
                    }
                }
                __syncthreads();
            }
        for (int r = tid; r < T; r += CLP_NT) { const int w = kw[r]; const double x = sCh[w].last; sCh[w].rank = r; sCand[r] = ClSL{x, exp(x - Lhi)}; }
        __syncthreads();                                                // (the plan records' LDS is free again)
    }
    if (tid == 0) sCand[T] = ClSL{PC_HUGE, 0.0};
    // where the two sorted sequences interleave (by key: snapshot points before candidates at a tie): for every candidate the snapshot points below
    // it (strictly: the logL test; or equal: its place in the order of deaths), for the snapshot points that can die in this launch (<= T deaths:
    // indices 0 .. T) the candidates below them; and the exponential of every death the launch can make
    for (int w = tid; w < T; w += CLP_NT) {
        const unsigned long long kc = d2key(sCh[w].last);
        {   // the first rank among the candidates of MY value (exact ties are real: a chain whose slices all fail returns its seed point, and two such
            // chains -- or such a chain and the live point it started from -- hold the same logL): `c_t > Lg_t` is a statement about values, so the
            // accepted candidates that count against it are those of rank >= this one, not >= my own
            int lo = 0, hi = T;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (d2key(sCand[mid].L) < kc) lo = mid + 1; else hi = mid; }
            sCh[w].rank |= lo << 16;
        }
        int lo = 0, hi = nlv;                                          // first snapshot index with key >= kc
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (d2key(sSort[mid].L) < kc) lo = mid + 1; else hi = mid; }
        belowS[w] = (unsigned short)lo;
        hi = nlv;                                                      // first snapshot index with key > kc
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (d2key(sSort[mid].L) <= kc) lo = mid + 1; else hi = mid; }
        belowE[w] = (unsigned short)lo;
    }
    for (int i = tid; i <= T && i <= NS; i += CLP_NT) {
        const unsigned long long ks = d2key(sSort[i].L);
        int lo = 0, hi = T;                                            // first candidate rank with key >= ks
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (d2key(sCand[mid].L) < ks) lo = mid + 1; else hi = mid; }
        rxS[i] = (unsigned short)lo;
        sSort[i].e = exp(sSort[i].L - Lhi);
    }
    // the candidates' table: entry s < Ncap = the point that occupied slot s when the lists were made, entry Ncap + w = the last baby of chain w;
    // cluster + 1 (0: not alive at any step of this launch), step of birth + 1 (0: alive when the launch begins), step of death (CLP_NEVER: none)
    for (int s = tid; s < Ncap; s += CLP_NT) tag[s] = (sS[s].o == -1 && sS[s].c >= 0) ? clp_tag(sS[s].c, 0, CLP_NEVER) : 0u;
    for (int c = tid; c <= S.B; c += CLP_NT) { const int sl = c < S.B ? sCS[c] : -1; tag[Ncap + c] = (sl >= 0 && sS[sl].o == c && sS[sl].c >= 0) ? clp_tag(sS[sl].c, 0, CLP_NEVER) : 0u; }
    {   // The nursery's records and the cross-volume matrix were written by other XCDs: touch what the launch will read, in bulk
        auto touch = [&](const void *base, size_t bytes) {
            const char *b = (const char *)base;
            int acc = 0;
            for (size_t o0 = (size_t)tid * 64; o0 < bytes; o0 += (size_t)CLP_NT * 64 * 8) {
                int v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const size_t o = o0 + (size_t)u * CLP_NT * 64; v[u] = (o < bytes) ? *(const volatile int *)(b + o) : 0; }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc ^= v[u];
            }
            asm volatile("" :: "v"(acc));
        };
        if (pass == 0) {
            touch(S.baby_logL, sizeof(double) * (size_t)T * nr);
            touch(S.nn_list, sizeof(int) * (size_t)T * nr * PC_NN_K);
        }
        // the cross-volume matrix in linear space about X_max^2, in the scratch half behind it: wave 1 asks for a row a death, and the exponential
        // of that row was a third of its time per death
        { double *xlinM = S.XpXq + (size_t)maxc * maxc;
          for (int e0 = tid; e0 < nc * nc; e0 += 4 * CLP_NT) {
              double v[4]; size_t at[4];
#pragma unroll
              for (int u = 0; u < 4; ++u) { const int e = e0 + u * CLP_NT; const bool in = e < nc * nc; at[u] = in ? (size_t)(e / nc) * maxc + e % nc : 0; v[u] = in ? S.XpXq[at[u]] : 0.0; }
#pragma unroll
              for (int u = 0; u < 4; ++u) if (e0 + u * CLP_NT < nc * nc) xlinM[at[u]] = exp(v[u] - 2.0 * lxm0); } }
    }
    if (tid == 0) { lp_prog = T; lp_done = 0; lp_stop = -2; lp_lists = T; pa_hard = 0x7fffffff; pa_end = 0x7fffffff; pa_jupd = 0x7fffffff; }
    const int curC_init = cl_uni((sSlotOf[0] != 0xFFFFu && sSort[0].L < PC_HUGE) ? sS[sSlotOf[0] != 0xFFFFu ? sSlotOf[0] : 0].c : 0);
    __syncthreads();
    const long long cyc0 = clock64();
    if (tid == 0) ctl->gen_cyc[1] += cyc0 - t_pass;                   // (developer counters: [1] staging, [0] the decisions, [2] behind the loop, [3] the whole kernel)

    // ------------------------------------------------------------------ phase A (wave 0): the acceptance vector, 64 steps at a time
    // steps that can be consumed at all: the nursery, a pass made again up to the chain wave 2 named, nothing when max_ndead = 0
    int Tp0 = T;
    if (redo_limit != CL_NO_LIMIT) Tp0 = T - 1 - redo_limit;
    if (hard_cap < Tp0) Tp0 = hard_cap;
    if (S.max_ndead == 0) Tp0 = 0;
    if (Tp0 < 0) Tp0 = 0;
    if (wv == 0) {
        __builtin_amdgcn_s_setprio(2);
        int Tp = Tp0, kprev = 0;
        long long walks = 0, fallbacks = 0;
        // Q of the settled steps: accepted candidates of rank >= r
        auto qprev = [&](int r) -> int { const int wd = r >> 6; return wd >= 16 ? 0 : sufW[wd + 1] + __popcll(accW[wd] >> (r & 63)); };
        int force_res0 = -3;                                          // step 0's last baby, identified by the full search (see the head of this file)
        for (int t0 = 0; t0 < Tp; t0 += 64) {
            const int t = t0 + lane; const bool in = t < Tp; const int w = in ? T - 1 - t : 0;
            const ClChain ch = sCh[w];
            const bool okv = in && ch.epoch == epoch0 && ch.last == ch.last;       // (a chain seeded before the cluster list changed is lost, nested_sampling.F90:313; a NaN is never above a contour)
            const int rk = in ? (ch.rank & 0xFFFF) : 0x7fff, rk_lo = in ? (ch.rank >> 16) : 0x7fff, ca = ch.ca;
            // ---- the logL test: slack of `snapshot points below me > Q(t, my rank)` after the settled steps
            const int sown = okv ? (int)belowS[w] - qprev(rk_lo) : 0;
            const int own_kind = !okv || sown <= 0 ? 0 : (sown > 63 ? 1 : 2);      // never / whatever the chunk does / depends on the chunk
            // ---- the last baby's candidates
            int ck[PC_NN_K], ccl[PC_NN_K], cthr[PC_NN_K], csig[PC_NN_K], cdyn[PC_NN_K];      // kind (0 dead, 1 alive, 2 depends on the chunk), cluster, rank threshold, slack, lane whose acceptance it needs (-1)
            {
                const int4 *L4 = (const int4 *)(S.nn_list + ((size_t)w * nr + (nr - 1)) * PC_NN_K);
                int4 a4 = make_int4(PC_NN_NONE, PC_NN_NONE, PC_NN_NONE, PC_NN_NONE), b4 = a4;
                if (own_kind) { a4 = L4[0]; b4 = L4[1]; walks++; }
                const int codes[PC_NN_K] = { a4.x, a4.y, a4.z, a4.w, b4.x, b4.y, b4.z, b4.w };
                bool cut = false;                                      // behind the first candidate that lives whatever happens nothing matters
#pragma unroll
                for (int k = 0; k < PC_NN_K; ++k) {
                    const int code = codes[k];
                    int kind = 0, cl = -1, thr = 0x7fff, sig = 0, dyn = -1;
                    if (!cut && own_kind && code != PC_NN_NONE) {
                        const int v = -(code + 1);                   // (chain index when code < 0)
                        const unsigned ix = code >= 0 ? (unsigned)code : (unsigned)(Ncap + v);
                        const unsigned tg = ix < (unsigned)(Ncap + S.B) ? tag[ix] : 0u;
                        const int tv = T - 1 - v;                     // the step of chain v in this pass
                        if (code < 0 && v < T) {
                            // the last baby of a chain of THIS pass: alive at my step iff accepted before it and not among the dead since
                            if (tv < t) {
                                const ClChain cv = sCh[v];
                                cl = cv.ca; thr = cv.rank & 0xFFFF;
                                const bool settled = tv < t0;
                                if (settled ? (tg != 0u) : (cv.epoch == epoch0)) {
                                    sig = (int)belowE[v] - qprev(cv.rank & 0xFFFF);
                                    kind = sig < 0 ? 0 : ((settled && sig > 63) ? 1 : 2);
                                    dyn = settled ? -1 : tv - t0;
                                }
                            }
                        } else if (tg != 0u) {
                            // a point of the snapshot (a slot's occupant of T0 still in place, or the last baby of a chain of an earlier launch)
                            cl = (int)(tg & 255u) - 1;
                            const int slot = code >= 0 ? code : sCS[v];
                            const int ix_s = (int)idxOf[slot];
                            if (ix_s >= Tp || ix_s > T) kind = 1;    // (at most Tp deaths: it cannot be among them)
                            else { thr = rxS[ix_s]; sig = ix_s - qprev(thr); kind = sig < 0 ? 0 : (sig > 63 ? 1 : 2); }
                        }
                    }
                    if (kind == 1) cut = true;
                    ck[k] = kind; ccl[k] = cl; cthr[k] = thr; csig[k] = sig; cdyn[k] = dyn;
                }
            }
            // ---- the chunk's ranks >= each threshold, as 64-bit masks (only for what depends on the chunk)
            unsigned mlo[PC_NN_K + 1], mhi[PC_NN_K + 1]; bool any_dyn[PC_NN_K + 1];
#pragma unroll
            for (int k = 0; k <= PC_NN_K; ++k) {
                const bool mine = k < PC_NN_K ? ck[k] == 2 : own_kind == 2;
                const int thr = k < PC_NN_K ? cthr[k] : rk_lo;
                any_dyn[k] = __ballot(mine) != 0ull;
                unsigned lo = 0u, hi = 0u;
                if (any_dyn[k]) {
                    const int th = mine ? thr : 0x7fffffff;
#pragma unroll 8
                    for (int s = 0; s < 32; ++s) { const int rs = __builtin_amdgcn_readlane(rk, s); lo |= (rs >= th) ? (1u << s) : 0u; }
#pragma unroll 8
                    for (int s = 0; s < 32; ++s) { const int rs = __builtin_amdgcn_readlane(rk, s + 32); hi |= (rs >= th) ? (1u << s) : 0u; }
                }
                mlo[k] = lo; mhi[k] = hi;
            }
            // ---- the fixed point over the chunk
            const unsigned lt_lo = lane < 32 ? ((1u << lane) - 1u) : 0xFFFFFFFFu, lt_hi = lane < 32 ? 0u : ((1u << (lane - 32)) - 1u);
            unsigned long long A = 0ull;
            int res = -2; bool okL = false;
            for (int it = 0; it < 80; ++it) {
                const unsigned alo = (unsigned)A & lt_lo, ahi = (unsigned)(A >> 32) & lt_hi;
                okL = own_kind == 1 || (own_kind == 2 && sown > (int)(__popc(alo & mlo[PC_NN_K]) + __popc(ahi & mhi[PC_NN_K])));
                res = -2;
#pragma unroll
                for (int k = PC_NN_K - 1; k >= 0; --k) {
                    bool alive = ck[k] == 1;
                    if (any_dyn[k] && ck[k] == 2) {
                        alive = csig[k] >= (int)(__popc(alo & mlo[k]) + __popc(ahi & mhi[k]));
                        if (cdyn[k] >= 0) alive = alive && ((A >> cdyn[k]) & 1ull);
                    }
                    res = alive ? ccl[k] : res;
                }
                if (t == 0 && force_res0 != -3) res = force_res0;
                const unsigned long long An = __ballot(okv && okL && res == ca);
                if (An == A) break;
                A = An;
            }
            // ---- a last baby no list resolves: the pass ends in front of its step (at step 0 the staged state IS the live set of its step)
            const unsigned long long hard = __ballot(okv && okL && res == -2);
            if (hard) {
                const int th = __ffsll((long long)hard) - 1;
                if (t0 + th == 0 && force_res0 == -3) {
                    fallbacks++;
                    force_res0 = cl_uni(full_search(T - 1, nr - 1));
                    if (force_res0 == -2) force_res0 = -1;
                    t0 -= 64;                                          // (this chunk again, the answer in hand)
                    continue;
                }
                Tp = t0 + th;
                A &= (th == 0) ? 0ull : ((1ull << th) - 1ull);
                if (lane == 0) atomicMin(&pa_hard, Tp);
            }
            // ---- settle the chunk: counts, the order of its acceptances, the bitmap of accepted ranks
            const bool acc = ((A >> lane) & 1ull) && t < Tp;
            const int kt = kprev + __popcll(A & ((1ull << lane) - 1ull));
            if (t < Tp) kAcc[t] = (unsigned short)kt;
            if (acc) {
                stepOf[kt] = (unsigned short)t;
                tag[Ncap + w] = clp_tag(ca, t + 1, CLP_NEVER);
                atomicOr(&accW[rk >> 6], 1ull << (rk & 63));
            }
            for (int l = 0; l < 17; ++l) {
                const int cnt = __popcll(__ballot(acc && (rk >> 6) >= l));
                if (cnt == 0) break;
                if (lane == l) sufW[l] += cnt;
            }
            kprev += __popcll(A);                                      // (lanes behind the last decided step never accept)
        }
        if (lane == 0) { kAcc[Tp] = (unsigned short)kprev; pa_Tp = Tp; pa_K = kprev; ctl->nn_walks += walks; ctl->nn_fallbacks += fallbacks; }
        __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    long long tq = cyc0;
#define CLP_MARK(i) do { if (tid == 0) { const long long now_ = clock64(); ctl->dbg[i] += now_ - tq; tq = now_; } } while (0)
    CLP_MARK(0);                                                      // (developer counters, PC_DEBUG=4: [0] phase A, [1] order of deaths + slots, [2] counts + volumes, [3] the volume sum + phantom masks, [4] prefix sums + commit, [5] waves 1-3, [6] write back, [7] passes)
    // ------------------------------------------------------------------ phase B (all waves): what the consumed chains leave behind
    const int Tp = pa_Tp, K = pa_K;
    // A cluster that loses its last point (delete_cluster, run_time_info.f90:507-598) used to end the pass: restaging for the rest of the nursery, ~120
    // times a 10-D Rastrigin run.  Under the engine's rule for chains in flight nothing in the rest of the pass depends on the deletion itself: the
    // cluster can neither gain nor lose a point any more, the chains seeded in it are lost from the next step on (what the remap does to them), its
    // volume leaves the update trigger's sum behind the step of its death -- and the arrays are compacted when the pass is over, cluster after cluster
    // in the order they ended.  (The reference farm's rule, settings.epoch_discard = 1: the pass ends at the death, as before.)
    const bool can_cont = !S.epoch_discard && !(S.ablate & PC_ABL_CL_END_AT_DEATH) && ctl->ncluster_dead + nc + 2 <= S.maxc_dead;
    auto qall = [&](int r) -> int { const int wd = r >> 6; return wd >= 16 ? 0 : sufW[wd + 1] + __popcll(accW[wd] >> (r & 63)); };
    // ---- B1: the order of deaths = the first K (+ 1) entries of the merge of the snapshot and the accepted candidates
    for (int t = tid; t < Tp; t += CLP_NT) {
        const int w = T - 1 - t;
        if (kAcc[t + 1] != kAcc[t]) { const int r = sCh[w].rank & 0xFFFF; const int pos = (int)belowE[w] + (K - qall(r)); if (pos <= K) sU[pos] = (unsigned short)(0x8000 | t); }
    }
    for (int i = tid; i <= K && i < nlv; i += CLP_NT) { const int pos = i + (K - qall(rxS[i])); if (pos <= K) sU[pos] = (unsigned short)i; }
    __syncthreads();
    // ---- B2: every death: who, from which slot (a newcomer's: the slot of the death it was accepted at), in which cluster; every step's contour
    for (int j = tid; j < K; j += CLP_NT) {
        const int tj = stepOf[j], wj = T - 1 - tj;
        const unsigned u = sU[j];
        int cd, code; double eL; unsigned short lk = 0xFFFFu, sd = 0xFFFFu;
        if (u & 0x8000u) { const int tb = (int)(u & 0x7FFFu), wb = T - 1 - tb; cd = sCh[wb].ca; eL = sCand[sCh[wb].rank & 0xFFFF].e; lk = kAcc[tb]; code = Ncap + wb; }
        else { const int sl = sSlotOf[u]; sd = (unsigned short)sl; cd = sS[sl].c; eL = sSort[u].e; const int o = sS[sl].o; code = o == -1 ? sl : Ncap + o; }
        link[j] = lk; slotD[j] = sd; cdca[j] = (unsigned short)(cd | (sCh[wj].ca << 8));
        sEvt[wj].eL = eL;
        tag[code] = (tag[code] & 0x0007FFFFu) | ((unsigned)tj << 19);     // (its step of death; it is alive AT that step)
    }
    for (int t = tid; t <= Tp && t < T; t += CLP_NT) {
        const unsigned u = sU[kAcc[t]];
        sHead[T - 1 - t].contour = (u & 0x8000u) ? sCh[T - 1 - (int)(u & 0x7FFFu)].last : sSort[u].L;
    }
    __syncthreads();
    // ---- B3: pointer jumping over "who died for whom"
    for (int round = 0; round < 11; ++round) {
        unsigned short nl[(1024 + CLP_NT - 1) / CLP_NT], ns[(1024 + CLP_NT - 1) / CLP_NT];
#pragma unroll
        for (int u = 0; u < (1024 + CLP_NT - 1) / CLP_NT; ++u) {
            const int j = tid + u * CLP_NT;
            nl[u] = 0xFFFFu; ns[u] = 0xFFFFu;
            if (j < K) { const unsigned short l = link[j]; ns[u] = slotD[j]; if (l != 0xFFFFu) { const unsigned short l2 = link[l]; if (l2 == 0xFFFFu) ns[u] = slotD[l]; else nl[u] = l2; } }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < (1024 + CLP_NT - 1) / CLP_NT; ++u) { const int j = tid + u * CLP_NT; if (j < K) { link[j] = nl[u]; slotD[j] = ns[u]; } }
        __syncthreads();
    }
    CLP_MARK(1);
    // ---- B4: a cluster's live count at each death = its count at launch + the additions - the deaths before it.  64 consecutive deaths to a wavefront
    //          (lane = death): inside the group the earlier deaths / additions of one's cluster are bit counts of two ballots per cluster id that
    //          occurs in the group; the groups before contribute their per-cluster totals (a table of byte pairs).  No pair loop over the deaths.
    const int nchunk = (K + 63) >> 6;
    for (int e = tid; e < nchunk * CL_MAXC; e += CLP_NT) ctot[e] = 0;
    __syncthreads();
    for (int c = wv; c < nchunk; c += CLP_NT / 64) {
        const int j = c * 64 + lane; const bool in = j < K;
        const unsigned me = in ? cdca[j] : 0xFFFFu; const int cd = (int)(me & 255u), ca = (int)(me >> 8);
        bool dD = !in, dA = !in;
        int inD_cd = 0, inA_cd = 0, inD_ca = 0, inA_ca = 0;
        const unsigned long long lt = (1ull << lane) - 1ull, le = lt | (1ull << lane);
        for (;;) {
            const unsigned long long todo = __ballot(!dD || !dA);
            if (!todo) break;
            const int pl = __ffsll((long long)todo) - 1;
            const int x = __builtin_amdgcn_readlane(dD ? ca : cd, pl);      // (the first lane with something left: its cluster of death, else of addition)
            const unsigned long long md = __ballot(in && cd == x), ma = __ballot(in && ca == x);
            if (cd == x) { inD_cd = __popcll(md & lt); inA_cd = __popcll(ma & lt); dD = true; }
            if (ca == x) { inD_ca = __popcll(md & le); inA_ca = __popcll(ma & lt); dA = true; }      // (deaths up to AND including mine: the count behind my own death)
            if (lane == 0) ctot[c * CL_MAXC + x] = (unsigned short)(__popcll(md) | (__popcll(ma) << 8));
        }
        if (in) sEvt[T - 1 - (int)stepOf[j]].b = (unsigned)inD_cd | ((unsigned)inA_cd << 8) | ((unsigned)inD_ca << 16) | ((unsigned)inA_ca << 24);
    }
    if (wv == CLP_NT / 64 - 1) {
        double a = 0.0;
        for (int j = 0; j < (CL_MAXC + 63) / 64; ++j) { const int q = lane + 64 * j; a += (q < nc) ? clX0[q] : 0.0; }
        const double s0 = wave_sum<4>(a);
        if (lane == 0) pa_sum0 = s0;
    }
    __syncthreads();
    unsigned short *dstart = (unsigned short *)kmin;                       // [CL_MAXC + 1] where a cluster's deaths begin, the deaths taken cluster by cluster (kmin's LDS: unused between staging and write back)
    int my_r[(1024 + CLP_NT - 1) / CLP_NT]; double my_rat[(1024 + CLP_NT - 1) / CLP_NT];
#pragma unroll
    for (int u = 0; u < (1024 + CLP_NT - 1) / CLP_NT; ++u) {
        const int j = tid + u * CLP_NT; my_r[u] = 0;
        if (j < K) {
            const unsigned me = cdca[j]; const int cd = (int)(me & 255u), ca = (int)((me >> 8) & 127u), c = j >> 6;
            const int wj = T - 1 - (int)stepOf[j];
            const unsigned pk = sEvt[wj].b;
            int Dd = (int)(pk & 255u), Ad = (int)((pk >> 8) & 255u), Da = (int)((pk >> 16) & 255u), Aa = (int)(pk >> 24);
            for (int c2 = 0; c2 < c; ++c2) { const unsigned a = ctot[c2 * CL_MAXC + cd], b = ctot[c2 * CL_MAXC + ca]; Dd += (int)(a & 255u); Ad += (int)(a >> 8); Da += (int)(b & 255u); Aa += (int)(b >> 8); }
            const int nd = clN0[cd] + Ad - Dd, na = clN0[ca] + Aa - Da;
            my_r[u] = Dd;                                                  // my place among my cluster's deaths
            sEvt[wj].b = (unsigned)nd | ((unsigned)na << 16);
            my_rat[u] = (double)nd * srcp[nd + 1];
            if (nd - 1 == 0 && cd != ca) {                                 // a cluster died (delete_cluster)
                if (can_cont) { clDead[cd] = (int)stepOf[j]; cdca[j] = (unsigned short)(me | 0x8000u); }
                else atomicMin(&pa_end, 2 * (int)stepOf[j] + 1);           // ... and the pass ends behind this step
            }
        }
    }
    if (wv == 0) {
        // where each cluster's deaths begin: exclusive prefix over the clusters of their totals (two clusters a lane)
        int t0 = 0, t1 = 0;
        for (int c2 = 0; c2 < nchunk; ++c2) { t0 += (int)(ctot[c2 * CL_MAXC + 2 * lane] & 255u); t1 += (int)(ctot[c2 * CL_MAXC + 2 * lane + 1] & 255u); }
        int inc = t0 + t1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
        dstart[2 * lane] = (unsigned short)(inc - t0 - t1); dstart[2 * lane + 1] = (unsigned short)(inc - t1);
        if (lane == 63) dstart[CL_MAXC] = (unsigned short)inc;
    }
    __syncthreads();
    // the deaths' volume ratios n / (n + 1) cluster by cluster, each cluster's in the order of its deaths ...
#pragma unroll
    for (int u = 0; u < (1024 + CLP_NT - 1) / CLP_NT; ++u) { const int j = tid + u * CLP_NT; if (j < K) { my_r[u] += (int)dstart[cdca[j] & 255u]; ratD[my_r[u]] = my_rat[u]; } }
    __syncthreads();
    // ... and the cluster's volume at each of its deaths: the product of the ratios of its deaths so far -- a thread a cluster, walking ITS deaths in
    // their order (the serial kernel's multiplications in its order); what the death moves the sum of the volumes by takes the ratio's place
    if (tid < CL_MAXC) {
        const int s0 = dstart[tid], s1 = dstart[tid + 1];
        double XL = clX0[tid];
        int r = s0;
        for (; r + 4 <= s1; r += 4) {
            const double r0 = ratD[r], r1 = ratD[r + 1], r2 = ratD[r + 2], r3 = ratD[r + 3];
            const double x0 = XL * r0, x1 = x0 * r1, x2 = x1 * r2, x3 = x2 * r3;
            ratD[r] = x0 - XL; ratD[r + 1] = x1 - x0; ratD[r + 2] = x2 - x1; ratD[r + 3] = x3 - x2;
            XL = x3;
        }
        for (; r < s1; ++r) { const double x0 = XL * ratD[r]; ratD[r] = x0 - XL; XL = x0; }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < (1024 + CLP_NT - 1) / CLP_NT; ++u) { const int j = tid + u * CLP_NT; if (j < K) sHead[T - 1 - (int)stepOf[j]].postXs = ratD[my_r[u]]; }      // (the running sum takes its place below)
    __syncthreads();
    CLP_MARK(2);
    const double UT = exp(ctl->logX_last_update + S.log_cf - lxm0);      // update trigger: sum_p X_p <= X_last_update * compression_factor
    if (wv == 0) {
        // the sum of the clusters' volumes behind every death, in the order of the deaths (the serial kernel's additions in its order)
        double s = pa_sum0;
        for (int j0 = 0; j0 < K; j0 += 64) {
            const int j = j0 + lane; const int wj = j < K ? T - 1 - (int)stepOf[j] : 0;
            const double dl = j < K ? sHead[wj].postXs : 0.0;
            const int dropv = (j < K && (cdca[j] & 0x8000u)) ? 1 : 0;
            double mine = 0.0, mine2 = 0.0;
            const int n = K - j0 < 64 ? K - j0 : 64;
            for (int l = 0; l < n; ++l) {
                const double d = readlane_f64(dl, l);
                s += d; mine = (lane == l) ? s : mine;
                // (its last point gone, n = 1: the ratio is exactly 1/2, the volume that is left exactly -d; the update test of this step still
                //  sees it, nested_sampling.F90:321-339, the steps behind do not)
                if (__builtin_amdgcn_readlane(dropv, l)) s += d;
                mine2 = (lane == l) ? s : mine2;
            }
            if (j < K) { sHead[wj].postXs = mine; sHead[wj].logw = mine2; }      // (logw: the sum the steps BEHIND this death see; wave 1 writes the log weight there later)
        }
    }
    // ---- B5: the phantom masks: babies 1 .. nr-1 above the contour and inside the seed cluster's cell (run_time_info.f90:747-757).  One chain = one
    //          wavefront's work (lane = baby); the next chain's records are requested while this one's are looked at.  Step 0 here, while the LDS
    //          still holds the live set of that step (its babies may ask for the full search); the others next to waves 1 - 3, behind the commit
    struct PhLoad { double bl; int4 a4, b4; };
    auto ph_load = [&](int t, int m) -> PhLoad {
        const int w = T - 1 - t, i = m * 64 + lane, ic = i < nr ? i : nr - 1;
        PhLoad r;
        r.bl = S.baby_logL[(size_t)w * nr + ic];
        const int4 *L4 = (const int4 *)(S.nn_list + ((size_t)w * nr + ic) * PC_NN_K);
        r.a4 = L4[0]; r.b4 = L4[1];
        return r;
    };
    auto ph_word = [&](int t, int m, const PhLoad &q) {
        const int w = T - 1 - t, i = m * 64 + lane;
        const ClChain ch = sCh[w];
        if (ch.epoch != epoch0 || clDead[ch.ca & 127] < t) { if (lane == 0) masks[(size_t)w * nw + m] = 0ull; return; }
        const double Lg = sHead[w].contour;
        const bool need = (i < nr - 1) && (q.bl > Lg);
        const int codes[PC_NN_K] = { q.a4.x, q.a4.y, q.a4.z, q.a4.w, q.b4.x, q.b4.y, q.b4.z, q.b4.w };
        int res = -2;
#pragma unroll
        for (int k = PC_NN_K - 1; k >= 0; --k) {
            const int code = codes[k];
            const unsigned sgn = (unsigned)(code >> 31);
            const unsigned ix = ((unsigned)code ^ sgn) + ((unsigned)Ncap & sgn);
            const unsigned tg = tag[ix < (unsigned)(Ncap + S.B) ? ix : (unsigned)(Ncap + S.B)];
            const bool alive = (tg & 255u) != 0u && (int)((tg >> 8) & 0x7FFu) <= t && (int)(tg >> 19) >= t;
            res = alive ? (int)(tg & 255u) - 1 : res;
        }
        if (!need) res = -1;
        unsigned long long unres = __ballot(res == -2);
        if (unres) {
            if (t == 0) {                                              // (step 0: the staged state is the live set of this step)
                while (unres) {
                    const int bl_lane = __ffsll((long long)unres) - 1; unres &= unres - 1;
                    const int r = full_search(w, m * 64 + bl_lane);
                    if (lane == bl_lane) res = r;
                }
            } else if (lane == 0) atomicMin(&pa_hard, t);              // a pass must end in front of this step (CL_MEET)
        }
        const unsigned long long pm = __ballot(need && res == ch.ca);
        if (lane == 0) masks[(size_t)w * nw + m] = pm;
    };
    if (wv == CLP_NT / 64 - 1 && Tp > 0) for (int m = 0; m < nw; ++m) ph_word(0, m, ph_load(0, m));
    __syncthreads();
    CLP_MARK(3);
    // ---- B6: prefix sums over the steps: acceptances, failed spawns, valid chains | evaluations, those of chains that placed no point |
    //          consecutive failures (nested_sampling.F90:315-319: a counter that an acceptance resets)
    constexpr int SPT = (1024 + CLP_NT) / CLP_NT;                    // steps per thread (consecutive; index Tp <= 1024 -- the totals -- has an owner too)
    long long p1[SPT], p2[SPT]; int fl_r[SPT], fl_c[SPT];              // exclusive prefixes at my steps; (reset seen, failures) before my steps
    int st_acc[SPT], st_fs[SPT], st_valid[SPT], st_win[SPT]; double st_sum[SPT];
    {
        long long s1 = 0, s2 = 0; int fr = 0, fc = 0;
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            const int t = tid * SPT + u;
            p1[u] = s1; p2[u] = s2; fl_r[u] = fr; fl_c[u] = fc;
            st_acc[u] = st_fs[u] = st_valid[u] = st_win[u] = 0;
            if (t <= Tp && t < T) st_win[u] = sHead[T - 1 - t].contour > Lhi;      // the next death leaves the launch's window: new references (host relaunches)
            if (t < Tp) {
                const int w = T - 1 - t; const ClChain ch = sCh[w];
                const bool valid = ch.epoch == epoch0 && !(clDead[ch.ca & 127] < t), acc = kAcc[t + 1] != kAcc[t];
                const bool fs = valid && !(ch.last > sHead[w].contour);
                st_acc[u] = acc; st_fs[u] = fs; st_valid[u] = valid;
                s1 += (long long)acc | ((long long)fs << 12) | ((long long)valid << 24);
                s2 += (long long)ch.nlike | ((long long)((!valid || !acc) ? ch.nlike : 0) << 32);
                if (acc) { fr = 1; fc = 0; } else if (valid) fc++;
            }
        }
        // inclusive scan of the threads' totals across the wave, then across the waves
        long long i1 = s1, i2 = s2; int ir = fr, ic = fc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o1 = __shfl_up(i1, d), o2 = __shfl_up(i2, d); const int orr = __shfl_up(ir, d), oc = __shfl_up(ic, d);
            if (lane >= d) { i1 += o1; i2 += o2; if (!ir) { ic += oc; ir = orr; } }
        }
        if (lane == 63) { pa_scan[wv] = i1; pa_scan[CLP_NT / 64 + wv] = i2; pa_scan[2 * (CLP_NT / 64) + wv] = ((long long)ir << 32) | (unsigned)ic; }
        __syncthreads();
        long long b1 = 0, b2 = 0; int br = 0, bc = 0;                   // what the waves before mine add
        for (int q = 0; q < wv; ++q) {
            b1 += pa_scan[q]; b2 += pa_scan[CLP_NT / 64 + q];
            const long long f = pa_scan[2 * (CLP_NT / 64) + q]; const int qr = (int)(f >> 32), qc = (int)(unsigned)f;
            if (qr) { br = 1; bc = qc; } else bc += qc;
        }
        // exclusive prefix of my thread = the waves before + the lanes before
        const long long e1 = b1 + i1 - s1, e2 = b2 + i2 - s2;
        int er, ec;                                                    // (reset, count) of everything before my thread = (waves before) o (lanes before)
        { const int lr = __shfl_up(ir, 1), lc = __shfl_up(ic, 1);
          const int pr = lane ? lr : 0, pc = lane ? lc : 0;
          if (pr) { er = 1; ec = pc; } else { er = br; ec = bc + pc; } }
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            p1[u] += e1; p2[u] += e2;
            if (!fl_r[u]) { fl_c[u] += ec; fl_r[u] = er; }
        }
    }
    // ---- B7: the step that ends the pass.  Code 2 t: the pass stops IN FRONT of step t; 2 t + 1: BEHIND it (update, a cluster's death)
    const int ndead0 = ctl->ndead, nph0 = ctl->nphantom, failures0 = ctl->failures;
    const int nd_lim = S.max_ndead == 0 ? -0x7fffffff - 1 : (S.max_ndead > 0 ? S.max_ndead : 0x7fffffff);
    {
        int mine = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            const int t = tid * SPT + u;
            st_sum[u] = pa_sum0;
            if (t < Tp) {                                              // the sum of the clusters' volumes as this step leaves it
                const int kd = kAcc[t + 1];
                if (kd > 0) { const int tl = stepOf[kd - 1]; st_sum[u] = tl == t ? sHead[T - 1 - tl].postXs : sHead[T - 1 - tl].logw; }
            }
        }
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            const int t = tid * SPT + u;
            if (t > Tp) continue;
            const int acc_ex = (int)(p1[u] & 0xFFF), fs_ex = (int)((p1[u] >> 12) & 0xFFF);
            const int failures_t = fl_c[u] + (fl_r[u] ? 0 : failures0);
            bool stop = false;
            if (ndead0 + acc_ex + fs_ex >= nd_lim) stop = true;        // more_samples_needed (nested_sampling.F90:514-543): max_ndead
            if (failures_t > S.nfail) stop = true;                      // :239
            if (st_win[u]) stop = true;
            if (t < Tp && (st_acc[u] || st_fs[u]) && ndead0 + acc_ex + fs_ex >= S.Dcap) stop = true;      // (capacity: the error is raised below)
            if (stop) { mine = 2 * t; break; }
            // behind a consumed chain that was not lost: the update trigger (nested_sampling.F90:321) -- the sum of the clusters' volumes as the deaths up
            // to this step left it (a launch that begins below the trigger -- a cluster's end took its volume out of the sum -- updates behind its
            // first such chain, accepted or not)
            if (t < Tp && st_valid[u]) {
                if (st_sum[u] <= UT) { mine = 2 * t + 1; break; }
            }
        }
        if (mine != 0x7fffffff) atomicMin(&pa_end, mine);
        if (tid == 0) { atomicMin(&pa_end, 2 * Tp); if (pa_hard < 0x7fffffff) atomicMin(&pa_end, 2 * pa_hard); }
    }
    __syncthreads();
    const int end_code = pa_end, t_end = (end_code + 1) >> 1;            // steps 0 .. t_end - 1 are consumed
    const int i_nursery_end = T - t_end;
    if ((end_code & 1) && tid == (t_end - 1) / SPT) {
#pragma unroll
        for (int u = 0; u < SPT; ++u) if (u == (t_end - 1) % SPT) pa_sum_end = st_sum[u];      // (the sum behind the pass's last step: the records it was read from are about to be rewritten)
    }
    // ---- B8: commit.  Plan records (their phantom rows: behind the masks) and the records for the waves behind; the slots' new occupants; the clusters' counts
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const int t = tid * SPT + u;
        if (t >= Tp) continue;
        const int w = T - 1 - t;
        const ClChain ch = sCh[w];
        const int acc_ex = (int)(p1[u] & 0xFFF), fs_ex = (int)((p1[u] >> 12) & 0xFFF);
        ClHead hd{};
        hd.dead_idx = -1;
        ClEvt ev{0.0, 0u, 0u};
        if (t < t_end) {
            if (!st_valid[u]) hd.contour = S.logzero;
            else {
                hd.contour = sHead[w].contour; hd.ph_cuid = clUid[ch.ca];
                if (st_acc[u]) {
                    const int j = kAcc[t]; const int cd = (int)(cdca[j] & 255u), slot = slotD[j];
                    const unsigned uj = sU[j];
                    hd.dead_idx = ndead0 + acc_ex + fs_ex; hd.dead_cuid = clUid[cd]; hd.postXs = sHead[w].postXs;
                    if (uj & 0x8000u) hd.dead_src = -(1 + (T - 1 - (int)(uj & 0x7FFFu)));
                    else { const int src = sS[slot].src; hd.dead_src = src >= 0 ? -(1 + src) : slot; }
                    const unsigned un = sU[j + 1];                    // the cluster expected to lose the next point (a newcomer: -1)
                    const int predC = (un & 0x8000u) ? -1 : sS[sSlotOf[un]].c;
                    const unsigned b = sEvt[w].b;
                    ev = cl_evt(cd, predC, slot, (int)(b & 0xFFFFu), (int)(b >> 16), sEvt[w].eL);
                } else if (st_fs[u]) {
                    // failed spawn: the last baby is recorded as dead with zero weight (run_time_info.f90:781-785)
                    hd.dead_idx = ndead0 + acc_ex + fs_ex; hd.dead_src = -(1 + w); hd.logw = S.logzero; hd.postXs = 1.0; hd.zl = -1.0; hd.dead_cuid = 0xFFFFFFFFu;
                }
            }
        }
        // (a step's record is its own thread's to overwrite: the other steps' fields read above -- contour, postXs through kAcc / stepOf -- were read
        //  in front of the barrier before this loop)
        sHead[w] = hd; sEvt[w] = ev;
    }
    __syncthreads();
    for (int j = tid; j < K; j += CLP_NT) {
        const int tj = stepOf[j];
        if (tj >= t_end) continue;
        const int wj = T - 1 - tj; const unsigned me = cdca[j]; const int cd = (int)(me & 255u), ca = (int)((me >> 8) & 127u), slot = slotD[j];
        atomicAdd(&clAdd[cd], -1); atomicAdd(&clAdd[ca], 1); atomicMax(&clLastJ[cd], j);
        sCS[wj] = slot;
        const int tdie = (int)(tag[Ncap + wj] >> 19);                   // the newcomer's own death
        if (tdie >= t_end) {                                           // ... not inside this pass: the slot is its own when the pass ends
            sS[slot].c = ca; sS[slot].o = wj; sS[slot].src = wj; sL[slot] = sCh[wj].last;
        }
    }
    __syncthreads();
    if (tid < nc && clLastJ[tid] >= 0) { const unsigned uj = sU[clLastJ[tid]]; clThr[tid] = (uj & 0x8000u) ? sCh[T - 1 - (int)(uj & 0x7FFFu)].last : sSort[uj].L; }
    // ---- the pass's outcome (what wave 0 of k_consume_cl leaves in out_i / out_d)
    {
        // totals at t_end: taken from the thread that owns step t_end (index Tp: the block's totals)
        const int owner = t_end / SPT, u_own = t_end % SPT;
        const bool have = t_end < SPT * CLP_NT && tid == owner;
        if (have) {
            long long q1 = 0, q2 = 0; int qr = 0, qc = 0, o_acc = 0, o_fs = 0, o_win = 0;
#pragma unroll
            for (int u = 0; u < SPT; ++u) if (u == u_own) { q1 = p1[u]; q2 = p2[u]; qr = fl_r[u]; qc = fl_c[u]; o_acc = st_acc[u]; o_fs = st_fs[u]; o_win = st_win[u]; }
            const int acc_ex = (int)(q1 & 0xFFF), fs_ex = (int)((q1 >> 12) & 0xFFF);
            int status = PC_ST_RUNNING, error = PC_ERR_NONE, need_drop = 0, exit_top = 0;
            const int failures = qc + (qr ? 0 : failures0), ndead = ndead0 + acc_ex + fs_ex;
            double lx_last = ctl->logX_last_update;
            if (end_code & 1) {
                // behind step t_end - 1: update trigger (nested_sampling.F90:321), delete_cluster (:339)
                const int jl = kAcc[t_end] - 1;                        // the last death up to that step
                const double sum_e = pa_sum_end;
                const bool update = sum_e <= UT;
                const unsigned b = jl >= 0 ? sEvt[T - 1 - (int)stepOf[jl]].b : 0u; const unsigned me = jl >= 0 ? cdca[jl] : 0u;
                need_drop = (!can_cont && jl >= 0 && (int)stepOf[jl] == t_end - 1 && (int)(b & 0xFFFFu) - 1 == 0 && (int)(me & 255u) != (int)((me >> 8) & 127u)) ? 1 : 0;
                if (update) { lx_last = lxm0 + log(sum_e); status = PC_ST_UPDATE; }
            } else {
                // in front of step t_end, in the order of the serial loop's head
                bool more = true;
                if (S.max_ndead == 0) more = false;
                else if (S.max_ndead > 0 && ndead >= S.max_ndead) more = false;
                else if (redo_limit != CL_NO_LIMIT && i_nursery_end - 1 == redo_limit) more = false;
                if (!more || failures > S.nfail) status = PC_ST_DONE;
                else if (i_nursery_end == 0 || o_win || t_end == pa_hard || t_end == hard_cap) exit_top = 1;      // the nursery is empty / the window / a baby for the full search
                else if (t_end < Tp && (o_acc || o_fs) && ndead >= S.Dcap) { status = PC_ST_ERROR; error = PC_ERR_DEAD_CAP; }
                else exit_top = 1;
            }
            out_i[0] = status; out_i[1] = error; out_i[2] = i_nursery_end; out_i[3] = epoch0; out_i[4] = failures; out_i[5] = ndead; out_i[6] = nph0;
            out_i[7] = need_drop; out_i[8] = T - 1; out_i[9] = acc_ex > 0; out_i[10] = exit_top; out_i[12] = ((t_end == pa_hard || t_end == hard_cap) && !(end_code & 1)) ? 1 : 0;
            out_i[13] = t_end; out_i[14] = kAcc[t_end];            // ... and the deaths among them
            out_d[2] = lx_last;
            out_l[0] = (long long)(q2 & 0xFFFFFFFFll); out_l[1] = t_end; out_l[2] = (long long)(q2 >> 32);      // evaluations, chains, evaluations of chains that placed no point
        }
    }
    if (tid == 0) { lp_prog = i_nursery_end; lp_done = 1; ctl->gen_cyc[0] += clock64() - cyc0; }
    __syncthreads();
    CLP_MARK(4);

    // ------------------------------------------------------------------ phase C: update_evidence, the live evidence, the lists (waves 1, 2, 3 of k_consume_cl)
    auto cl_wait = [&](int w) -> bool { return lp_prog <= w; };       // (every decision is in place: a chain is either consumed or not)
#define CL_MEET() \
        __syncthreads(); \
        { const int stop_ = lp_stop, fin_ = out_i[2], hard_ = pa_hard, tend_ = out_i[13]; bool again_ = false; \
          if (S.use_prec && stop_ != -2 && redo_limit == CL_NO_LIMIT && stop_ > fin_ - 1) { \
              /* the precision criterion was met at a chain the decisions have gone past: nothing has left the LDS -- the pass again, up to that chain */ \
              redo_limit = stop_; again_ = true; } \
          if (hard_ < tend_) { \
              /* a phantom candidate of a consumed chain found no living entry in its list: the pass again, ending in front of that chain */ \
              hard_cap = hard_; again_ = true; } \
          if (again_) { __syncthreads(); pass--; continue; } }
    if (wv == 0) {
        CL_MEET();
        t_meet = clock64();
        {
            int status = out_i[0], i_nursery = out_i[2], failures = out_i[4], ndead = out_i[5], nph = out_i[6];
            const int need_drop = out_i[7], exit_top = out_i[10];
            long long nlike = ctl->nlike + out_l[0], niter = ctl->niter + out_l[1], nlike_failed = ctl->nlike_failed + out_l[2];
            const int stop = lp_stop;
            const bool prec_now = S.use_prec && stop != -2 && stop == i_nursery - 1;       // more_samples_needed fails before the next chain
            if (status == PC_ST_RUNNING && exit_top && prec_now) status = PC_ST_DONE;
            if (need_drop && status == PC_ST_RUNNING) {
                // A cluster died.  settings.epoch_discard: the administrator's epoch moves on (nested_sampling.F90:339-341) and what is left
                // of the nursery fails the guard of :313 -- after the loop's termination test, which sees the same state before each of them
                bool more = true;
                if (S.max_ndead == 0) more = false;
                else if (S.max_ndead > 0 && ndead >= S.max_ndead) more = false;
                else if (prec_now) more = false;
                if (!more || failures > S.nfail) status = PC_ST_DONE;
                else if (S.epoch_discard) {
                    double nl = 0.0;
                    for (int w = lane; w < i_nursery; w += 64) {
                        nl += (double)sCh[w].nlike;
                        ClHead h{}; h.dead_idx = -1; h.contour = S.logzero; sHead[w] = h;      // (their first phantom row: below, with everybody's)
                        for (int m = 0; m < nw; ++m) masks[(size_t)w * nw + m] = 0ull;
                    }
                    const long long tot = (long long)wave_sum<4>(nl);                 // (exact: counts far below 2^53)
                    nlike += tot; nlike_failed += tot; niter += i_nursery;
                    i_nursery = 0;
                }
            }
            if (lane == 0) {
                out_i[0] = status; out_i[2] = i_nursery;
                ctl->nlike = nlike; ctl->niter = niter; ctl->nlike_failed = nlike_failed;
            }
            for (int q = lane; q < nc; q += 64) { S.cl_n[q] = clN0[q] + clAdd[q]; S.death_thr[q] = clThr[q]; }
        }
    } else if (wv == 1) {
        // ================================================================ wave 1: update_evidence
        const double logZ0 = ctl->logZ, logZ20 = ctl->logZ2;
        double Xp[J], XL[J], Fl[J], Gl[J], Flog[J], Glog[J], ZX[J], kZX[J], rZX[J], k2a[J];
        double rZXmax = -PC_HUGE;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int q = lane + 64 * j; const bool in = q < nc;
            Xp[j] = in ? S.logXp[q] : -PC_HUGE; Fl[j] = 1.0; Gl[j] = 1.0; Flog[j] = 0.0; Glog[j] = 0.0;
            const double zx0 = in ? S.logZXp[q] : NEGBIG;
            rZX[j] = fmax(zx0, 2.0 * lxm0 + Lhi); ZX[j] = in ? exp(zx0 - rZX[j]) : 0.0; kZX[j] = exp(2.0 * lxm0 + Lhi - rZX[j]);
            if (in) rZXmax = fmax(rZXmax, rZX[j]);
        }
        rZXmax = wave_max(rZXmax);
        const double rZ = fmax(logZ0, lxm0 + Lhi), kZ = exp(lxm0 + Lhi - rZ);
        const double rZ2 = fmax(logZ20, fmax(rZXmax + Lhi, 2.0 * lxm0 + 2.0 * Lhi)), k2b = exp(2.0 * lxm0 + 2.0 * Lhi - rZ2);
        double Zl = exp(logZ0 - rZ), Z2l = exp(logZ20 - rZ2);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const bool in = lane + 64 * j < nc;
            XL[j] = in ? exp(Xp[j] - lxm0) : 0.0;
            k2a[j] = exp(rZX[j] + Lhi - rZ2);
        }
        double kZv = kZ, k2bv = k2b, lxm0v = lxm0;
        asm volatile("" : "+v"(kZv), "+v"(k2bv), "+v"(lxm0v));
        // the row of the cross-volume matrix for the cluster expected to lose a point next, in linear space about X_max^2
        // ... the rows of the deaths to come are requested THREE deaths ahead: every death of the pass is known by now, and a row comes from L2 in about
        // the time a death takes -- asked for one death ahead (as k_consume_cl must: it learns the next death from wave 0) the wave waited for it every
        // time.  Three row buffers with fixed roles (death g uses buffer g mod 3 and refills it for death g + 3: no register is copied while its load
        // is in flight), the deaths in groups of 63 so that the roles survive the groups' boundaries
        double rowA[J], rowB[J], rowC[J];
        const double *xlinM = S.XpXq + (size_t)maxc * maxc;                 // (made by this pass's staging)
        auto row_load = [&](double (&dst)[J], int c) {
#pragma unroll
            for (int j = 0; j < J; ++j) { const int q = lane + 64 * j; dst[j] = (q < nc) ? xlinM[(size_t)c * maxc + q] : 0.0; }
        };
        const int Kc = out_i[14];
        auto cd_vec = [&](int jbase) -> int {                                // the dying clusters of deaths jbase .. jbase + 63, a lane each
            const int jj = Kc > 0 ? (jbase + lane < Kc ? jbase + lane : Kc - 1) : 0;
            return Kc > 0 ? (int)((sEvt[T - 1 - (int)stepOf[jj]].a >> 1) & 127u) : 0;
        };
        const long long w1_t0 = clock64();
        int qcd_cur = cd_vec(0), qcd_nxt = cd_vec(63);
        row_load(rowA, __builtin_amdgcn_readlane(qcd_cur, 0)); row_load(rowB, __builtin_amdgcn_readlane(qcd_cur, 1)); row_load(rowC, __builtin_amdgcn_readlane(qcd_cur, 2));
        int any_death = 0;
        // a cluster's own accumulators <Z_p>, <Z_p^2>, <Z_p X_p> with their scales: lane = cluster, like everything else here (through the LDS record of
        // the dying cluster they were an 88-byte read and write a death by one lane)
        double Ozp[J], Ozp2[J], Ozpx[J], Okzp[J], Okp2a[J], Okp2b[J], Okzpx[J]; int Otouched[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int q = lane + 64 * j; const ClOwn o = sOwn[q < nc ? q : 0];
            Ozp[j] = o.zp; Ozp2[j] = o.zp2; Ozpx[j] = o.zpx; Okzp[j] = o.kzp; Okp2a[j] = o.kp2a; Okp2b[j] = o.kp2b; Okzpx[j] = o.kzpx; Otouched[j] = 0;
        }
        // (the deaths of the pass 63 at a time: lane l fetches everything death j0 + l asks of the LDS -- its record, log n, 1 / (n + 1) ... -- side by
        //  side with the other lanes, and the serial loop takes its operands by v_readlane instead of three dependent LDS round trips a death)
        for (int j0 = 0; j0 < Kc; j0 += 63) {
          const int jq = j0 + lane < Kc ? j0 + lane : Kc - 1;
          const int q_w = T - 1 - (int)stepOf[jq];
          const ClEvt q_ev = sEvt[q_w];
          const int q_nd = (int)(q_ev.b & 0xFFFFu);
          const double q_l0 = slogn[q_nd], q_l1 = slogn[q_nd + 1], q_l2 = slogn[q_nd + 2], q_r1 = srcp[q_nd + 1], q_r2 = srcp[q_nd + 2];
          const int nq = Kc - j0 < 63 ? Kc - j0 : 63;
          if (j0 > 0) { qcd_cur = qcd_nxt; qcd_nxt = cd_vec(j0 + 63); }
          auto death = [&](int lq, double (&row)[J]) __attribute__((always_inline)) {
            const int w = __builtin_amdgcn_readlane(q_w, lq);
            const unsigned ev_a = (unsigned)__builtin_amdgcn_readlane((int)q_ev.a, lq);
            const int cd = (int)((ev_a >> 1) & 127u), nd = __builtin_amdgcn_readlane(q_nd, lq);
            const double eL = readlane_f64(q_ev.eL, lq);
            const double l0 = readlane_f64(q_l0, lq), l1 = readlane_f64(q_l1, lq), l2 = readlane_f64(q_l2, lq), r1 = readlane_f64(q_r1, lq), r2 = readlane_f64(q_r2, lq);
            const double XLd = cl_get<J>(XL, cd), Fd = cl_get<J>(Fl, cd), Gd = cl_get<J>(Gl, cd), ZXd = cl_get<J>(ZX, cd), k2ad = cl_get<J>(k2a, cd);
            const double Xd = cl_get<J>(Xp, cd);
            const double rat = (double)nd * r1, c1 = eL * r1, c2 = eL * rat * r2;
            const double XXs = cl_get<J>(row, cd) * Gd;                  // <X_cd^2> now, about X_max^2
            const double logweight = Xd - l1;
            // ---- update_evidence (run_time_info.f90:211-296); every accumulation reads the state before the death
            const double tZ = XLd * c1;
            const double tXX = XXs * (eL * c1 * r2);                       // <X^2> L^2 / ((n+1)(n+2))
            Zl += tZ * kZv;                                                // <Z> += X L / (n+1)
            Z2l += 2.0 * (ZXd * c1 * k2ad + tXX * k2bv);                    // <Z^2> += 2 <Z X> L/(n+1) + 2 <X^2> L^2/((n+1)(n+2))
#pragma unroll
            for (int j = 0; j < J; ++j) {                                  // <Z X_q>, one cluster per lane
                const bool self = lane + 64 * j == cd;
                const double cross = row[j] * Fd * Fl[j] * c1 * kZX[j];
                ZX[j] = self ? ZX[j] * rat + XXs * c2 * kZX[j] : ZX[j] + cross;
            }
#pragma unroll
            for (int j = 0; j < J; ++j)                                    // the dying cluster's own accumulators
                if (lane + 64 * j == cd) {
                    const double zp_n = Ozp[j] + tZ * Okzp[j];
                    const double zp2_n = Ozp2[j] + 2.0 * (Ozpx[j] * c1 * Okp2a[j] + tXX * Okp2b[j]);
                    const double zpx_n = Ozpx[j] * rat + XXs * c2 * Okzpx[j];
                    Ozp[j] = zp_n; Ozp2[j] = zp2_n; Ozpx[j] = zpx_n; Otouched[j] = 1;
                }
            if (lane == 0) { sHead[w].logw = logweight; sHead[w].zl = Zl; }      // (the rest of the plan record was written with the decisions)
            // ---- the dying cluster: volume and the factors of its row of the cross-volume matrix
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (lane + 64 * j == cd) { Xp[j] += l0 - l1; Flog[j] += l0 - l1; Glog[j] += l0 - l2; XL[j] *= rat; Fl[j] *= rat; Gl[j] *= (double)nd * r2; }
            any_death = 1;
            // this buffer's next turn: the death three ahead
            { const int i3 = lq + 3;
              row_load(row, i3 < 63 ? __builtin_amdgcn_readlane(qcd_cur, i3 & 63) : __builtin_amdgcn_readlane(qcd_nxt, (i3 - 63) & 63)); }
          };
          for (int lq = 0; lq < nq; lq += 3) {
            death(lq, rowA);
            if (lq + 1 < nq) death(lq + 1, rowB);
            if (lq + 2 < nq) death(lq + 2, rowC);
          }
        }
        if (lane == 0) ctl->wave_cyc[0] += clock64() - w1_t0;
        CL_MEET();
#pragma unroll
        for (int j = 0; j < J; ++j) { const int q = lane + 64 * j; if (q < nc && Otouched[j]) { sOwn[q].zp = Ozp[j]; sOwn[q].zp2 = Ozp2[j]; sOwn[q].zpx = Ozpx[j]; sOwn[q].touched = 1; } }
        if (lane == 0) {
            out_d[0] = any_death ? cl_log(rZ, Zl, S.logzero) : logZ0; out_d[1] = any_death ? cl_log(rZ2, Z2l, S.logzero) : logZ20;
            out_d[4] = rZ;
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int q = lane + 64 * j;
            if (q < nc) { S.logXp[q] = Xp[j]; if (any_death) S.logZXp[q] = cl_log(rZX[j], ZX[j], S.logzero); Fbuf[q] = Flog[j]; Gbuf[q] = Glog[j]; }
        }
    } else if (wv == 2) {
        // ================================================================ wave 2: the live evidence and more_samples_needed
        const double logZ0 = ctl->logZ;
        double XL[J], lref[J], lsum[J], Eq[J], kd[J], rn[J]; int n[J];
        double R0 = -PC_HUGE;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int q = lane + 64 * j; const bool in = q < nc;
            n[j] = in ? clN0[q] : 0; lref[j] = in ? S.lse_ref[q] : -PC_HUGE; lsum[j] = in ? S.lse_sum[q] : 0.0;
            if (in && n[j] > 0) R0 = fmax(R0, lref[j]);
        }
        R0 = wave_max(R0);
        const double rZ = fmax(logZ0, lxm0 + Lhi), kZ = exp(lxm0 + Lhi - rZ);
        double Zl = exp(logZ0 - rZ);
        double acc = 0.0;
        {
            double b = 0.0;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int q = lane + 64 * j; const bool in = q < nc;
                XL[j] = in ? exp(S.logXp[q] - lxm0) : 0.0;
                Eq[j] = (in && n[j] > 0) ? exp(lref[j] - R0) : 0.0;
                kd[j] = in ? exp(Lhi - lref[j]) : 0.0;
                rn[j] = srcp[n[j]];                                        // (1 / n of every cluster in a register: two of them change a death, their new values come with the death's operands)
                b += (in && n[j] > 0) ? (lsum[j] * rn[j]) * XL[j] * Eq[j] : 0.0;
            }
            acc = wave_sum<4>(b);
        }
        double E0 = exp(S.log_prec + rZ - lxm0 - R0);              // more_samples_needed in linear space: acc < Zl * E0
        double kZv = kZ, Lhiv = Lhi, lxm0v = lxm0, lprec = S.log_prec, rZv = rZ;
        asm volatile("" : "+v"(kZv), "+v"(Lhiv), "+v"(lxm0v), "+v"(lprec), "+v"(rZv));
        asm volatile("" : "+v"(E0), "+v"(R0));
        const bool use_prec = S.use_prec != 0;
        // the criterion before the first chain of the launch, then behind every death
        bool stopped = false;
        if (use_prec && (!(acc > 0.0) || acc < Zl * E0)) { if (lane == 0) cl_lst(&lp_stop, T - 1); stopped = true; }
        const int Kc = out_i[14];
        const long long w2_t0 = clock64();
        for (int j0 = 0; j0 < Kc && !stopped; j0 += 64) {
          const int jq = j0 + lane < Kc ? j0 + lane : Kc - 1;
          const int q_w = T - 1 - (int)stepOf[jq];
          const ClEvt q_ev = sEvt[q_w];
          const ClChain q_ch = sCh[q_w];
          const ClSL q_me = sCand[q_ch.rank & 0xFFFF];                  // exp(Llast - Lhi), made with the ranks
          const double q_r1 = srcp[(int)(q_ev.b & 0xFFFFu) + 1];
          const int q_ndm = (int)(q_ev.b & 0xFFFFu) - 1;                  // the dying cluster's count behind the death, the receiving one's behind the addition: their reciprocals
          const double q_rd = srcp[q_ndm > 0 ? q_ndm : 0], q_ra = srcp[(int)(q_ev.b >> 16) + 1];
          const int nq = Kc - j0 < 64 ? Kc - j0 : 64;
          {   // (the sum over the clusters afresh, lane by lane, at the head of every group of deaths; inside a group it moves by what the dying and the
              //  receiving cluster changed -- a wave-wide sum a death was a quarter of this wave's time)
              double b = 0.0;
#pragma unroll
              for (int j = 0; j < J; ++j) b += (n[j] > 0) ? (lsum[j] * rn[j]) * XL[j] * Eq[j] : 0.0;
              acc = wave_sum<4>(b);
          }
          for (int lq = 0; lq < nq && !stopped; ++lq) {
            const int w = __builtin_amdgcn_readlane(q_w, lq);
            const unsigned ev_a = (unsigned)__builtin_amdgcn_readlane((int)q_ev.a, lq), ev_b = (unsigned)__builtin_amdgcn_readlane((int)q_ev.b, lq);
            const int cd = (int)((ev_a >> 1) & 127u), nd = (int)(ev_b & 0xFFFFu), ca = __builtin_amdgcn_readlane(q_ch.ca, lq), na = (int)(ev_b >> 16);
            const double eL = readlane_f64(q_ev.eL, lq);
            const double r1 = readlane_f64(q_r1, lq), rdm = readlane_f64(q_rd, lq), rap = readlane_f64(q_ra, lq);
            const double XLd = cl_get<J>(XL, cd), kdd = cl_get<J>(kd, cd);
            const double rat = (double)nd * r1, c1 = eL * r1;
            const double tZ = XLd * c1;
            Zl += tZ * kZv;                                                // <Z> += X L / (n+1), as wave 1 forms it
            const double e_del = eL * kdd;                                 // exp(L - lse_ref[cd])
            double t_old[J];                                               // my cluster's term of the sum before this death (it only matters in the two lanes that change)
#pragma unroll
            for (int j = 0; j < J; ++j) t_old[j] = (n[j] > 0) ? (lsum[j] * rn[j]) * XL[j] * Eq[j] : 0.0;
            bool rebased = false;
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (lane + 64 * j == cd) { XL[j] *= rat; n[j] = nd - 1; lsum[j] -= e_del; rn[j] = rdm; }
            // ---- add_point: the receiving cluster's log-sum-exp
            const double Llast = readlane_f64(q_ch.last, lq);
            const double lref_a = cl_get<J>(lref, ca), lsum_a = cl_get<J>(lsum, ca);
            const double me_e = readlane_f64(q_me.e, lq);
            double nref = lref_a, nsum, nEq = cl_get<J>(Eq, ca), nkd = cl_get<J>(kd, ca);
            if (na == 0 || Llast > lref_a) {                             // the cluster's reference moves to the newcomer (utils.F90 logsumexp bookkeeping)
                nsum = (na == 0) ? 1.0 : lsum_a * exp(lref_a - Llast) + 1.0;
                nref = Llast;
                if (nref - R0 > 600.0) {                                 // (cannot be represented about the launch's reference: re-base every cluster)
                    const double R1 = nref;
#pragma unroll
                    for (int j = 0; j < J; ++j) Eq[j] = (lane + 64 * j < nc && n[j] > 0) ? exp(lref[j] - R1) : 0.0;
                    E0 = exp(lprec + rZv - lxm0v - R1);
                    R0 = R1; rebased = true;
                }
                nEq = exp(nref - R0); nkd = exp(Lhiv - nref);            // (a newcomer may sit far above the window: no products of precomputed factors here)
            } else {
                // lsum + exp(Llast - lref): the product of the two precomputed factors where both are ordinary numbers
                const bool plain = fabs(Llast - Lhiv) < 600.0 && fabs(Lhiv - lref_a) < 600.0;
                nsum = lsum_a + (plain ? me_e * nkd : exp(Llast - lref_a));
            }
#pragma unroll
            for (int j = 0; j < J; ++j) if (lane + 64 * j == ca) { n[j] = na + 1; lref[j] = nref; lsum[j] = nsum; Eq[j] = nEq; kd[j] = nkd; rn[j] = rap; }
            if (rebased) {
                double b = 0.0;
#pragma unroll
                for (int j = 0; j < J; ++j) b += (n[j] > 0) ? (lsum[j] * rn[j]) * XL[j] * Eq[j] : 0.0;
                acc = wave_sum<4>(b);
            } else {
                double dlt[J];
#pragma unroll
                for (int j = 0; j < J; ++j) dlt[j] = ((n[j] > 0) ? (lsum[j] * rn[j]) * XL[j] * Eq[j] : 0.0) - t_old[j];
                acc += cl_get<J>(dlt, cd);
                if (ca != cd) acc += cl_get<J>(dlt, ca);
            }
            // more_samples_needed before the NEXT chain
            if (use_prec && (!(acc > 0.0) || acc < Zl * E0)) { if (lane == 0) cl_lst(&lp_stop, w - 1); stopped = true; }
          }
        }
        if (lane == 0) ctl->wave_cyc[1] += clock64() - w2_t0;
        {   // (the sum as it stands, afresh, for the estimate that leaves the kernel)
            double b = 0.0;
#pragma unroll
            for (int j = 0; j < J; ++j) b += (n[j] > 0) ? (lsum[j] * rn[j]) * XL[j] * Eq[j] : 0.0;
            if (!stopped) acc = wave_sum<4>(b);
        }
        CL_MEET();
        if (lane == 0) { const double v = acc > 0.0 ? log(acc) + lxm0 + R0 : S.logzero; out_d[3] = (v > S.logzero + 800.0) ? v : pc_logaddexp(S.logzero, v); }
#pragma unroll
        for (int j = 0; j < J; ++j) { const int q = lane + 64 * j; if (q < nc) { S.lse_ref[q] = lref[j]; S.lse_sum[q] = lsum[j]; } }
    } else if (wv == 3) {
        // ================================================================ wave 3: the clusters' lists
        // Engine rule (oracle keyed mode): a newcomer that replaces a death of its own cluster takes the dead point's position -- nothing
        // moves.  Otherwise the dying cluster's last entry fills the hole (delete_point, array_utils.f90:433-458) and the newcomer is
        // appended to its own cluster's list.
        const int Kc = out_i[14];
        const long long w3_t0 = clock64();
        for (int j0 = 0; j0 < Kc; j0 += 64) {
          const int jq = j0 + lane < Kc ? j0 + lane : Kc - 1;
          const int q_w = T - 1 - (int)stepOf[jq];
          const ClEvt q_ev = sEvt[q_w];
          const int q_ca = sCh[q_w].ca, q_cd = (int)((q_ev.a >> 1) & 127u);
          const int q_od = lstOff[q_cd], q_oa = lstOff[q_ca];
          const unsigned long long moved = __ballot(j0 + lane < Kc && q_cd != q_ca);      // (a death inside the newcomer's own cluster moves nothing)
          unsigned long long todo = moved;
          while (todo) {
            const int lq = __ffsll((long long)todo) - 1; todo &= todo - 1;
            const unsigned ev_a = (unsigned)__builtin_amdgcn_readlane((int)q_ev.a, lq), ev_b = (unsigned)__builtin_amdgcn_readlane((int)q_ev.b, lq);
            const int od = __builtin_amdgcn_readlane(q_od, lq), oa = __builtin_amdgcn_readlane(q_oa, lq);
            if (lane == 0) {
                const int slot = (int)(ev_a >> 16), nd = (int)(ev_b & 0xFFFFu), na = (int)(ev_b >> 16);
                const int p = sS[slot].p;
                const int last = lst[od + nd - 1];
                if (p != nd - 1) { lst[od + p] = last; sS[last].p = p; }
                lst[oa + na] = slot; sS[slot].p = na;
            }
          }
        }
        if (lane == 0) ctl->wave_cyc[2] += clock64() - w3_t0;
        CL_MEET();
    } else {
        // ================================================================ waves 4 ..: the phantom masks of the consumed chains (step 0's are made)
        const int npw = CLP_NT / 64 - 4, me4 = wv - 4;
        const long long w4_t0 = clock64();
        if (nw == 1) {
            int t = 1 + me4;
            PhLoad cur = ph_load(t < t_end ? t : 0, 0);
            while (t < t_end) {
                const int tn = t + npw;
                const PhLoad nxt = ph_load(tn < t_end ? tn : t, 0);   // (the last one asks for its own records again: no branch around a load)
                ph_word(t, 0, cur);
                cur = nxt; t = tn;
            }
        } else {
            for (int t = 1 + me4; t < t_end; t += npw) for (int m = 0; m < nw; ++m) ph_word(t, m, ph_load(t, m));
        }
        if (tid == 4 * 64) ctl->wave_cyc[3] += clock64() - w4_t0;
        CL_MEET();
    }
#undef CL_MEET
    __syncthreads();
    CLP_MARK(5);
    // ------------------------------------------------------------------ write back (all waves)
    int status = out_i[0];
    const int i_nursery = out_i[2], need_drop = out_i[7], seg_hi = out_i[8], hard_end = out_i[12];
    {   // the first phantom row of every consumed chain: a prefix sum over the masks' bit counts, in the order the chains were consumed
        const int ntot = T - i_nursery, tend = out_i[13], nph0 = out_i[6];      // (behind a cluster's death under epoch_discard the rest of the nursery is consumed too, with no phantoms)
        constexpr int SPT = (1024 + CLP_NT) / CLP_NT;
        int cnt[SPT], s = 0;
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            const int t = tid * SPT + u; cnt[u] = 0;
            if (t < tend) { const int w = T - 1 - t; for (int m = 0; m < nw; ++m) cnt[u] += __popcll(masks[(size_t)w * nw + m]); }
            s += cnt[u];
        }
        int inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
        if (lane == 63) pa_scan[wv] = inc;
        __syncthreads();
        int base = nph0, total = nph0;
        for (int q = 0; q < CLP_NT / 64; ++q) { if (q < wv) base += (int)pa_scan[q]; total += (int)pa_scan[q]; }
        int ex = base + inc - s;
#pragma unroll
        for (int u = 0; u < SPT; ++u) { const int t = tid * SPT + u; if (t < ntot) sHead[T - 1 - t].ph_base = t < tend ? ex : total; ex += cnt[u]; }
        if (tid == 0) { out_i[6] = total; if (total > S.Pcap && out_i[1] == PC_ERR_NONE) { out_i[0] = PC_ST_ERROR; out_i[1] = PC_ERR_PHANTOM_CAP; } }
        __syncthreads();
        status = out_i[0];
    }
    int epoch = out_i[3];
    const double rZ = out_d[4];
    for (int s = tid; s < Ncap; s += CLP_NT) {
        const ClSlot r = sS[s];
        S.live_logL[s] = sL[s]; S.live_cluster[s] = r.c; S.live_pos[s] = r.p; S.nn_slot_owner[s] = r.o; S.slot_src[s] = r.src;
        if (r.c >= 0) S.cl_list[(size_t)r.c * Ncap + r.p] = s;
    }
    for (int c = tid; c < S.B; c += CLP_NT) S.nn_chain_slot[c] = sCS[c];
    for (int c = tid; c < nc; c += CLP_NT) {
        const ClOwn o = sOwn[c];
        if (o.touched) { S.logZp[c] = cl_log(o.rzp, o.zp, S.logzero); S.logZp2[c] = cl_log(o.rzp2, o.zp2, S.logzero); S.logZpXp[c] = cl_log(o.rzpx, o.zpx, S.logzero); }
    }
    // the cross-volume matrix picks up the factors of the launch's deaths: X_p X_q *= f_p f_q, X_p^2 *= g_p
    for (int e0 = tid; e0 < nc * nc; e0 += 4 * CLP_NT) {               // (four entries in flight per thread: the loads before the stores)
        double v[4], add[4]; size_t at[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * CLP_NT; const bool in = e < nc * nc;
            const int p = in ? e / nc : 0, q = in ? e % nc : 0;
            at[u] = (size_t)p * maxc + q; add[u] = !in ? 0.0 : ((p == q) ? Gbuf[p] : Fbuf[p] + Fbuf[q]);
            v[u] = S.XpXq[at[u]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) if (add[u] != 0.0) S.XpXq[at[u]] = v[u] + add[u];
    }
    // plan records of the chains this launch consumed
    for (int w = i_nursery + tid; w <= seg_hi; w += CLP_NT) {
        const ClHead r = sHead[w];
        PcPlanHead h;
        h.dead_idx = r.dead_idx; h.dead_src = r.dead_src; h.ph_base = r.ph_base; h.dead_cuid = r.dead_cuid; h.ph_cuid = r.ph_cuid; h.ph_count = 0;
        h.logw = r.logw; h.contour = r.contour;
        const bool spawn_failed = r.zl < 0.0;
        h.postX = spawn_failed ? 0.0 : ref_d[1]; h.postXs = r.postXs;
        h.postZ = spawn_failed ? 0.0 : cl_log(rZ, r.zl, S.logzero);
        if (h.dead_idx < 0) { h.dead_src = 0; h.dead_cuid = 0u; h.logw = 0.0; h.postX = 0.0; h.postXs = 1.0; h.postZ = 0.0; }
        *(PcPlanHead *)&S.plan[w] = h;
        for (int m = 0; m < nw; ++m) S.plan[w].ph_mask[m] = masks[(size_t)w * nw + m];
    }
    // find_min_loglikelihoods (run_time_info.f90:883-909), once: lowest (logL, list position) of every cluster
    for (int c = tid; c < CL_MAXC; c += CLP_NT) { kmin[c] = KEY_HUGE; lstOff[c] = 0x7fffffff; }
    __syncthreads();
    for (int s = tid; s < Ncap; s += CLP_NT) if (sS[s].c >= 0) atomicMin(&kmin[sS[s].c], d2key(sL[s]));
    __syncthreads();
    for (int s = tid; s < Ncap; s += CLP_NT) if (sS[s].c >= 0 && d2key(sL[s]) == kmin[sS[s].c]) atomicMin(&lstOff[sS[s].c], sS[s].p);
    __syncthreads();
    for (int s = tid; s < Ncap; s += CLP_NT) { const ClSlot r = sS[s]; if (r.c >= 0 && d2key(sL[s]) == kmin[r.c] && r.p == lstOff[r.c]) { S.imin_slot[r.c] = s; S.logLp[r.c] = sL[s]; } }
    for (int c = tid; c < nc; c += CLP_NT) if (kmin[c] == KEY_HUGE) { S.imin_slot[c] = -1; S.logLp[c] = PC_HUGE; }
    __syncthreads();
    int ncd = ctl->ncluster_dead, cluster_deleted = 0;
    const int tend_wb = out_i[13];
    for (int drop = 0; drop < CL_MAXC; ++drop) {
        // delete_cluster (run_time_info.f90:507-598): the clusters that lost their last point in the consumed steps leave one after the other, in the order
        // they ended (the others keep theirs) -- or, where the pass ended AT a cluster's death (need_drop), that one: the first empty cluster
        __threadfence_block();
        __syncthreads();
        int p = -1;
        if (need_drop) { if (drop == 0) for (int c = 0; c < nc && p < 0; ++c) if (S.cl_n[c] == 0) p = c; }
        else { int best = CLP_ALIVE; for (int c = 0; c < nc; ++c) { const int dc = clDead[c]; if (dc < tend_wb && dc < best) { best = dc; p = c; } } }
        if (p < 0) break;
        {
            if (tid == 0 && ncd < S.maxc_dead) { S.logZp_dead[ncd] = S.logZp[p]; S.logZp2_dead[ncd] = S.logZp2[p]; S.cl_uid_dead[ncd] = S.cl_uid[p]; }
            __syncthreads();
            ncd++;
            {
                const int m1 = nc - 1;
                constexpr int NV = (CL_MAXC * CL_MAXC + CLP_NT - 1) / CLP_NT;
                double v[NV];
#pragma unroll
                for (int u = 0; u < NV; ++u) {
                    const int e = tid + u * CLP_NT;
                    if (e < m1 * m1) { const int na = e / m1, nb = e % m1; v[u] = S.XpXq[(size_t)(na + (na >= p)) * maxc + nb + (nb >= p)]; }
                }
                double t[9]; int ti[2]; unsigned tu = 0u;
                const int c = p + tid;
                if (c < m1) {
                    t[0] = S.logLp[c + 1]; t[1] = S.logXp[c + 1]; t[2] = S.logZp[c + 1]; t[3] = S.logZXp[c + 1]; t[4] = S.logZp2[c + 1]; t[5] = S.logZpXp[c + 1];
                    t[6] = S.lse_ref[c + 1]; t[7] = S.lse_sum[c + 1]; t[8] = S.death_thr[c + 1]; ti[0] = S.cl_n[c + 1]; ti[1] = S.imin_slot[c + 1]; tu = S.cl_uid[c + 1];
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < NV; ++u) {
                    const int e = tid + u * CLP_NT;
                    if (e < m1 * m1) S.XpXq[(size_t)(e / m1) * maxc + e % m1] = v[u];
                }
                if (c < m1) {
                    S.logLp[c] = t[0]; S.logXp[c] = t[1]; S.logZp[c] = t[2]; S.logZXp[c] = t[3]; S.logZp2[c] = t[4]; S.logZpXp[c] = t[5];
                    S.lse_ref[c] = t[6]; S.lse_sum[c] = t[7]; S.death_thr[c] = t[8]; S.cl_n[c] = ti[0]; S.imin_slot[c] = ti[1]; S.cl_uid[c] = tu;
                }
            }
            {   // Cholesky factors and covariance matrices: groups of clusters whose elements fit sixteen to a thread
                const int DD = D * D;
                int G = (16 * CLP_NT) / DD; if (G < 1) G = 1;
                for (int c0 = p; c0 < nc - 1; c0 += G) {
                    const int g = (nc - 1 - c0 < G) ? nc - 1 - c0 : G, tot = g * DD;
                    for (int e0 = 0; e0 < tot; e0 += 16 * CLP_NT) {               // (one pass unless a single matrix exceeds the share)
                        double a[16], b[16];
#pragma unroll
                        for (int u = 0; u < 16; ++u) { const int e = e0 + tid + u * CLP_NT; if (e < tot) { a[u] = S.chol[(size_t)(c0 + 1) * DD + e]; b[u] = S.cov[(size_t)(c0 + 1) * DD + e]; } }
                        __syncthreads();
#pragma unroll
                        for (int u = 0; u < 16; ++u) { const int e = e0 + tid + u * CLP_NT; if (e < tot) { S.chol[(size_t)c0 * DD + e] = a[u]; S.cov[(size_t)c0 * DD + e] = b[u]; } }
                        if (tot > 16 * CLP_NT) __syncthreads();                   // (the next pass reads what this one's neighbours write)
                    }
                }
            }
            for (int s = tid; s < Ncap; s += CLP_NT) if (sS[s].c > p) { sS[s].c -= 1; S.live_cluster[s] = sS[s].c; }
            __syncthreads();
            // (the lists of the clusters behind the deleted one move up a row)
            for (int s = tid; s < Ncap; s += CLP_NT) if (sS[s].c >= p) S.cl_list[(size_t)sS[s].c * Ncap + sS[s].p] = s;
            if (S.epoch_discard) epoch++;
            else {
                // the engine's rule (oracle: remap_chains): the chains seeded in the cluster that ended are lost, the others stay in the
                // nursery -- the clusters behind p moved up one place and the chains seeded in them follow
                for (int w = tid; w < i_nursery; w += CLP_NT) {
                    const int c = S.ch_cluster[w];
                    if (c == p) { S.ch_cluster[w] = -1; S.ch_epoch[w] = -1; }
                    else if (c > p) S.ch_cluster[w] = c - 1;
                }
            }
            {   // (the steps at which the clusters behind it ended move up with them)
                const int v = (tid >= p && tid + 1 < CL_MAXC) ? clDead[tid + 1] : CLP_ALIVE;
                __syncthreads();
                if (tid >= p && tid < CL_MAXC) clDead[tid] = v;
            }
            nc--; cluster_deleted = 1;
            if (nc == 0) status = PC_ST_DONE;
        }
    }
    if (pass == 0) seg_hi_launch = seg_hi;
    CLP_MARK(6);
    if (tid == 0) { ctl->dbg[7] += 1; if (hard_end) ctl->nn_fallbacks += 1; }      // (a pass that ended in front of a baby for the full search: PCHIP_PATH_NN_FALLBACKS)
    if (tid == 0) {
        if (t_meet) ctl->gen_cyc[2] += clock64() - t_meet;
        ctl->status = status; ctl->error = out_i[1]; ctl->i_nursery = i_nursery; ctl->admin_epoch = epoch; ctl->failures = out_i[4];
        ctl->ncluster = nc; ctl->ncluster_dead = ncd; ctl->ndead = out_i[5]; ctl->nphantom = out_i[6];
        ctl->seg_hi = seg_hi_launch; ctl->seg_lo = i_nursery; ctl->cluster_deleted = cluster_deleted;
        ctl->logZ = out_d[0]; ctl->logZ2 = out_d[1]; ctl->logX_last_update = out_d[2]; ctl->live_logZ = out_d[3];
    }
    // go round again?  (uniform: every thread holds the same values) -- behind a cluster's death, or in front of a baby that asks for the full search
    const bool again = ((cluster_deleted && need_drop) || hard_end) && status == PC_ST_RUNNING && i_nursery > 0 && !(S.epoch_discard && cluster_deleted) && nc >= 2 && out_i[1] == PC_ERR_NONE &&
                       ncd + nc + 2 <= S.maxc_dead && pass < 1024 && (!(S.ablate & PC_ABL_CL_END_AT_DEATH) || !cluster_deleted);
    if (!again) break;
    redo_limit = CL_NO_LIMIT; hard_cap = 0x7fffffff;
    __threadfence(); __syncthreads();                 // the state this pass wrote is what the next one stages
    clp_sort_live(S, smem);
    __threadfence(); __syncthreads();
    }
    __syncthreads();
    if (tid == 0) ctl->gen_cyc[3] += clock64() - t_start;            // (developer counters: staging, decisions, behind them, whole kernel)
#undef CLP_MARK
    pc_publish_ctl(S);
