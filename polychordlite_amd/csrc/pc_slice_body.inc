// pc_slice_body.inc -- the body of k_slice (pc_sample.hip), included by the one-run kernel and by k_slice_many (several runs in
// step, blockIdx.y = run) so that both are the same statements on `S`, `batch`, `phi_lds`, `mat_lds`.  Not a header: no include guard.
    PC_DYN_LDS(smem);                              // (a quadratic-form source, shared values: behind the form's front block -- pc_sample.hip)
    __builtin_amdgcn_s_setprio(LEAN == 2 ? 0 : 3);  // a chain is one long dependent instruction stream: it goes first on its SIMD
#if defined(SLICE_DBG) && SLICE_DBG == 2
    const long long kc0 = clock64(), kw0 = wall_clock64();
#endif
    // (FW > 0 with WPB = 4: four chains a workgroup AND their four helper wavefronts -- waves 0 .. 3 the chains, waves 4 .. 7 their helpers, so that
    //  every SIMD of the compute unit gets one chain: see `helped` below)
    constexpr bool HELPED = FW > 0 && WPB == 4 && (LEAN == 1 || LEAN == 3 || LEAN == 5);
    const int lane = threadIdx.x & 63, wv = (WPB > 1) ? (int)((threadIdx.x >> 6) & (HELPED ? 3 : 0xFF)) : 0, chain = blockIdx.x * WPB + wv;
    const size_t per_wave = ((size_t)S.D + S.nr + (phi_lds || LEAN == 1 ? (size_t)S.nr * (S.D + 1) : 0) + (FW > 0 ? (size_t)FW * S.D + (size_t)S.nr * (S.D + 2) : 0) + (HELPED ? (size_t)((S.nr + 3) / 4) * 128 + (size_t)S.nr : 0) + 1) & ~(size_t)1;   // doubles
    double *ybuf = (double *)smem + (size_t)wv * per_wave;   // [D] (corr gaussian only)
    int *sdeck = (int *)(ybuf + S.D);              // [nr] deck, only used when nr > 64
    int *sj = sdeck + S.nr;                        // [nr]
    double *tbuf = ybuf + S.D + S.nr;              // [nr][D+1] theta of every baby (when it fits: phi_lds)
    double *Mlds = (double *)smem + (size_t)WPB * per_wave;  // [D][D] inverse covariance, transposed (mat_lds), shared
    const int D = S.D, nr = S.nr, nT = S.nT;
    const double logzero = S.logzero;
    // LEAN (the metric configuration's shape: built-in Gaussian by its closed form along the chord, derived parameters through LDS, the
    // deck in registers, one grade, keyed draws): the kernel's other variants are compiled out -- same statements, a third of the code,
    // and the wave-uniform state fits the scalar registers (the general kernel spills ~100 of them into vector lanes and reads them back
    // with v_readlane, each with its hazard slots, all through the slice loop)
    // LEAN = 2: BASELINE configs[4]'s shape -- the correlated Gaussian with M.s of every direction made on the matrix cores (msp), no
    // derived parameters, the deck in LDS (num_repeats > 64), no matrix in LDS.
    // LEAN = 3 / 4: the Rastrigin function / the twin Gaussian (BASELINE configs[2] / [3]) evaluated as device functors, everything else
    // as LEAN = 1 leaves it where it applies (one grade, keyed draws, no correlated Gaussian).
    // LEAN = 5: the built-in Gaussian as a device functor (settings.ablate bit 0: one wave reduction per trial, no closed form along the chord) with the
    // same treatment the Rastrigin and twin-Gaussian functors get -- the figure a user's own device functor can expect (bench.py value_general_functor).
    constexpr bool lean = LEAN == 1, lean2 = LEAN == 2, leanf = LEAN == 3 || LEAN == 4 || LEAN == 5, lean_any = LEAN != 0;
    constexpr int KINDV = LEAN == 3 ? PC_LIKE_RASTRIGIN : (LEAN == 4 ? PC_LIKE_TWIN_GAUSSIAN : (LEAN == 5 ? PC_LIKE_GAUSSIAN : -1));
    const bool seq_mode = !lean_any && SPECIAL && S.seq_mode != 0, graded = !lean_any && SPECIAL && S.ngrade > 1;
    if (lean) phi_lds = 1;
    if (lean2) { phi_lds = 0; mat_lds = 0; }
    // Round 6: a chain's HELPER wavefront (fused lean variants launched with 128 threads a chain: pc_launch_slice_fused).  A wavefront alone
    // on its SIMD issues an instruction every 5-6 cycles whatever the dependences, and the chip has as many SIMDs again as a nursery has
    // chains: what does not depend on the seed -- the deck's shuffle, the whitening of the chain's directions (one cluster: its factor is
    // cluster 0's) -- is another wavefront's instruction stream, next to the seed choice and the start point instead of in front of them.
    // The two meet at ONE barrier; the helper ends there.  Same statements, same order per quantity: same numbers.
    // (two wavefronts a workgroup -- chain, helper -- put the chains of a compute unit on two of its four SIMDs, two to a SIMD: 15.3 ms a run
    //  against 11.8.  Eight wavefronts -- four chains, then their four helpers -- give every SIMD one of each.)
    constexpr bool helped = HELPED;
    const int role = helped ? (int)(threadIdx.x >> 8) : 0;

    LaneDims<DPL> ld;
    int slot, seed_cluster = 0;
    double contour;
    // FW: the loads of the whitening prologue are issued first -- raw direction `lane` (+64, ...) and the Cholesky factor of
    // cluster 0 (the seed's cluster unless there are several) -- and travel while the seed is chosen and the deck shuffled
    constexpr int FWN = FW > 0 ? FW : 1;
    constexpr int FWL = FW > 0 ? (FW * FW + 63) / 64 : 1;
    double vv0[FWN], Lpre[FWL];
    auto preload_whitening = [&](int cl) __attribute__((always_inline)) {
        const double *rawc = S.nhat_raw + (size_t)chain * S.nb_total * D * D;
#pragma unroll
        for (int d = 0; d < FWN; ++d) vv0[d] = (d < D && lane < nr) ? rawc[(size_t)lane * D + d] : 0.0;
        const double *Lg = S.chol + (size_t)cl * D * D;
#pragma unroll
        for (int q = 0; q < FWL; ++q) { const int e = lane + 64 * q; Lpre[q] = (e < D * D) ? Lg[e] : 0.0; }
    };
    if constexpr (FW > 0) { if (!helped || role == 1) preload_whitening(0); }
    // the deck and the whitening as functions: the chain's own wavefront calls them below, or its helper does here
    const bool deck_in_regs = lean || (!lean2 && nr <= 64);
    auto shuffle_deck_regs = [&](unsigned long long seq_g0) __attribute__((always_inline)) -> int {
        if constexpr (FW > 0) {
            // (drawn ahead with the bases on the side stream, k_nhats<.., 1>: there under its tag, or not)
            if (!seq_mode) {
                const int *rec = pc_deck_record(S, chain);
                const unsigned long long tg = pc_deck_tag(S, batch, chain, nr);
                const int dk = rec[2 + lane];
                if (__builtin_amdgcn_readfirstlane((int)(rec[0] == (int)(unsigned)tg && rec[1] == (int)(unsigned)(tg >> 32)))) return dk;
            }
        }
        PC_DECK_SHUFFLE(dk, S, batch, chain, lane, nr, seq_mode, seq_g0)       // (pc_seed.h: one text with the records' writers)
        return dk;
    };
    // (one wavefront's LDS traffic: ordered by issue; the workgroup barrier where the chain has no helper -- as it always was -- and a
    //  compiler fence where it has one, whose only barrier is the meeting point)
    auto lds_order = [&]() __attribute__((always_inline)) { if (helped) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else __syncthreads(); };
    // (qcT_: the closed form's s.M.s of every direction, LEAN = 1 with a helper -- the sum over the coordinates in the order of the chain's wave
    //  butterfly, a balanced tree over each row of sixteen, rows left to right, as pc_slice_t.hip restates it: the same bits the chain would
    //  reduce to at the head of the direction's slice, here for all directions at once, a lane each, ~60 instructions)
    auto whiten_all = [&](double *Lsh, double *nhs_, double *wsh_, double *qcT_, const double *spn_) __attribute__((always_inline)) {
        if constexpr (FW > 0) {
#pragma unroll
            for (int q = 0; q < FWL; ++q) { const int e = lane + 64 * q; if (e < FW * D) Lsh[e] = Lpre[q]; }
            lds_order();                                                    // one wave per workgroup
            const double *rawc = S.nhat_raw + (size_t)chain * S.nb_total * D * D;   // direction v (generation order) at + v * D
            for (int v0 = 0; v0 < nr; v0 += 64) {
                const int v = v0 + lane;
                if (v < nr) {
                    double vv[FWN], t[FWN];
#pragma unroll
                    for (int d = 0; d < FWN; ++d) { vv[d] = (v0 == 0) ? vv0[d] : ((d < D) ? rawc[(size_t)v * D + d] : 0.0); t[d] = 0.0; }
#pragma unroll
                    for (int bb = 0; bb < FWN; ++bb)
#pragma unroll
                        for (int aa = bb; aa < FWN; ++aa) t[aa] += Lsh[(size_t)aa * D + bb] * vv[bb];
#pragma unroll
                    for (int aa = 0; aa < FWN; ++aa) if (aa >= D) t[aa] = 0.0;
                    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
#pragma unroll
                    for (int d = 0; d < FWN; d += 4) { p0 += t[d] * t[d]; p1 += t[d + 1] * t[d + 1]; p2 += t[d + 2] * t[d + 2]; p3 += t[d + 3] * t[d + 3]; }
                    const double wn = sqrt((p0 + p1) + (p2 + p3)), iw = 1.0 / wn;
#pragma unroll
                    for (int d = 0; d < FWN; ++d) if (d < D) nhs_[(size_t)v * (D + 1) + d] = t[d] * iw;
                    wsh_[v] = wn * 3.0;
                    if constexpr (LEAN == 1) {
                        if (qcT_) {
#pragma clang fp contract(off)
                            double z2[FWN];
#pragma unroll
                            for (int d = 0; d < FWN; ++d) { const double zB = ((d < D ? spn_[d] : 0.0) * (t[d] * iw)) * S.like.inv_sigma; z2[d] = zB * zB; }
                            double rs[(FWN + 15) / 16];
#pragma unroll
                            for (int r = 0; r < (FWN + 15) / 16; ++r) {
                                double q4[4];
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const int b0 = 16 * r + 4 * q;
                                    const double e0 = b0 < FWN ? z2[b0 < FWN ? b0 : 0] : 0.0, e1 = b0 + 1 < FWN ? z2[b0 + 1 < FWN ? b0 + 1 : 0] : 0.0;
                                    const double e2 = b0 + 2 < FWN ? z2[b0 + 2 < FWN ? b0 + 2 : 0] : 0.0, e3 = b0 + 3 < FWN ? z2[b0 + 3 < FWN ? b0 + 3 : 0] : 0.0;
                                    q4[q] = (e0 + e1) + (e2 + e3);
                                }
                                rs[r] = (q4[0] + q4[1]) + (q4[2] + q4[3]);
                            }
                            qcT_[v] = (FWN <= 16) ? rs[0] : rs[0] + rs[(FWN + 15) / 16 - 1];
                        }
                    }
                }
            }
            lds_order();
        }
    };
    if constexpr (FW > 0) {
        if (role == 1) {
            // ---- the helper: deck, whitening (one cluster), the meeting point, the end
            double *tbuf_h = ybuf + S.D + S.nr;
            double *Lsh = tbuf_h + (phi_lds ? (size_t)nr * (D + 1) : 0), *nhs_ = Lsh + (size_t)FW * D, *wsh_ = nhs_ + (size_t)nr * (D + 1);
            const int dk = shuffle_deck_regs(0ull);
            if (lane < nr) sdeck[lane] = dk;
            const int one = S.ctl->ncluster == 1 ? 1 : 0;
            double *U = wsh_ + nr, *qcT_ = U + (size_t)((nr + 3) / 4) * 128;
            if (LEAN == 1 && lane < D) ybuf[lane] = (S.prior.hi ? S.prior.hi[lane] : 1.0) - (S.prior.lo ? S.prior.lo[lane] : 0.0);      // (the box's sides: ld.span of the chain's lanes)
            if (one) whiten_all(Lsh, nhs_, wsh_, LEAN == 1 ? qcT_ : nullptr, ybuf);
            if (lane == 0) { sj[0] = one; sj[1] = 0; }
            __syncthreads();
            // ... and, while the chain samples, the uniforms of its slices 4, 5, ... (one Philox call a lane covers four slices; the chain makes its
            // first four itself and finds the others here: a hundred instructions a group off its own stream)
            for (int g = 1; g < (nr + 3) / 4; ++g) {
                const uint32_t sl = (uint32_t)(4 * g) + (uint32_t)(lane >> 4);
                double a_, b_;
                pc_uniform2(S.k0, S.k1, PC_DOM_SLICE, batch, (uint32_t)chain, (sl * PC_SLICE_STRIDE) / 2 + (uint32_t)(lane & 15), a_, b_);
                U[((size_t)g * 64 + lane) * 2] = a_; U[((size_t)g * 64 + lane) * 2 + 1] = b_;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) __hip_atomic_store(&sj[1], g, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            return;
        }
    }
    if constexpr (FW > 0) {
        int sel = 0, sl = 0;
        select_seed_wave(S, batch, chain, lane, sel, sl);      // GenerateSeed (generate.F90:19-55), nested_sampling.F90:267-273
        if (lane == 0) {
            S.ch_cluster[chain] = sel; S.ch_seed_slot[chain] = sl;
            S.ch_contour[chain] = S.logLp[sel];                      // nested_sampling.F90:270
            S.ch_epoch[chain] = S.ctl->admin_epoch;
            if (chain == 0) { S.ctl->i_nursery = gridDim.x * WPB; S.ctl->batch_id = batch; }
        }
        seed_cluster = __builtin_amdgcn_readfirstlane(sel); slot = __builtin_amdgcn_readfirstlane(sl);
        contour = S.logLp[seed_cluster];
    } else { slot = S.ch_seed_slot[chain]; contour = S.ch_contour[chain]; }
#if defined(SLICE_DBG) && SLICE_DBG == 2
    const long long kp1 = clock64();
#endif
    double x0[DPL];
    {
        const double *seed = S.live + (size_t)slot * nT;
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const int dim = lane + 64 * k;
            ld.on[k] = dim < D;
            const double lo = (PT == 0 && ld.on[k] && S.prior.lo) ? S.prior.lo[dim] : 0.0;
            const double hi = (PT == 0 && ld.on[k] && S.prior.hi) ? S.prior.hi[dim] : 1.0;
            ld.lo[k] = lo; ld.span[k] = hi - lo;
            ld.mean[k] = (ld.on[k] && S.like.mean) ? S.like.mean[dim] : 0.0;
            x0[k] = ld.on[k] ? seed[dim] : 0.5;
        }
    }
    // pool mode: the babies land in this chain's rows of the phantom array; none of them is a phantom before the chain is consumed
    if (S.pool) for (int i = lane; i < nr; i += 64) S.ph_cuid[(size_t)S.pool_base + (size_t)chain * nr + i] = PC_CUID_NONE;
#if defined(SLICE_DBG) && SLICE_DBG == 2
    const long long kp2 = clock64();
#endif
    // PT: the chain's prior table, its constants read once (pc_table_load); every trial is then cube -> theta by pc_table_theta and a
    // likelihood call -- no closed form along the chord, no carried products of the correlated Gaussian
    ChainCtx<DPL, NROWS, PT> C{S, ld, lane, ybuf, 0, false, 0.0, 0.0, 0.0, 0.0};
    if constexpr (PT != 0) PC_PRIOR_LOAD(DPL, PT == 2, S, lane, C.tb);
#ifdef PCHIP_USER_TERMS
    // the terms form of a source: the second theta of eval_pair behind the chain's block, where the launchers add nDims doubles for it
    // (pc_terms_lds); the sum of every baby in the spare double of its tbuf row (the rows are D + 1 apart).  Several sums
    // (PCHIP_USER_SUMS): a block of their own behind the second theta, [nr][PC_NSUMS], there when phi_lds is set (the launchers count it
    // in that decision: pc_slice_phi_lds) -- the D + 1 stride of tbuf, of the bases and of the Cholesky staging stays what it is
#pragma unroll
    for (int k = 0; k < PC_NSUMS; ++k) C.tsum[k] = 0.0;
    C.ybuf2 = (double *)smem + (size_t)WPB * per_wave;
#ifdef PCHIP_USER_SUMS
    double *sums_lds = C.ybuf2 + S.D;
#endif
#endif
    const bool corr = PT == 0 && (lean2 || (!lean && !leanf && S.like.kind == PC_LIKE_CORR_GAUSSIAN));
    C.quad = PT == 0 && !leanf && (lean_any || ((corr || S.like.kind == PC_LIKE_GAUSSIAN) && !(S.ablate & PC_ABL_FUNCTOR)));
    C.qnorm = corr ? -((double)D * PC_LOG_TWO_PI + S.like.logdetcov) / 2.0 : S.like.norm;
    // correlated Gaussian: y = theta - mean and M.y travel with the chain (updated, not recomputed, at every
    // accepted point); the matrix is read from LDS when it fits
    const double *Mt = S.like.invcov;             // transposed: Mt[b*D + a] = M(a,b), lanes read consecutive a
    double yv[DPL], My[DPL], sv[DPL], Ms[DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) { yv[k] = 0.0; My[k] = 0.0; sv[k] = 0.0; Ms[k] = 0.0; }
    auto matvec = [&](const double (&vec)[DPL], double (&out)[DPL]) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) if (ld.on[k]) ybuf[lane + 64 * k] = vec[k];
        __syncthreads();                             // one wave per workgroup
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const int a = lane + 64 * k;
            double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
            if (ld.on[k]) {
                int b = 0;
                for (; b + 3 < D; b += 4) {
                    t0 += Mt[(size_t)b * D + a] * ybuf[b]; t1 += Mt[(size_t)(b + 1) * D + a] * ybuf[b + 1];
                    t2 += Mt[(size_t)(b + 2) * D + a] * ybuf[b + 2]; t3 += Mt[(size_t)(b + 3) * D + a] * ybuf[b + 3];
                }
                for (; b < D; ++b) t0 += Mt[(size_t)b * D + a] * ybuf[b];
            }
            out[k] = (t0 + t1) + (t2 + t3);
        }
        __syncthreads();
    };
    // msp: M.s of every direction and M.y of the start point were formed by k_nhats_q on the matrix cores (nhat_Ms, ch_My):
    // no matrix here at all; y and M.y are carried along the chords for the whole chain (a rounding error per slice, the
    // size of the one a direct evaluation makes)
    const bool msp = lean2 || (!lean && !leanf && corr && S.nhat_Ms != nullptr && C.quad);
    double Ms_next[DPL];
#pragma unroll
    for (int k = 0; k < DPL; ++k) Ms_next[k] = 0.0;
    if (corr) {
        if (mat_lds) {
            for (int e = threadIdx.x; e < D * D; e += 64 * WPB) Mlds[e] = S.like.invcov[e];
            __syncthreads();
            Mt = Mlds;
        }
#pragma unroll
        for (int k = 0; k < DPL; ++k) yv[k] = ld.on[k] ? (ld.lo[k] + ld.span[k] * x0[k]) - ld.mean[k] : 0.0;
        if (msp) {
#pragma unroll
            for (int k = 0; k < DPL; ++k) My[k] = ld.on[k] ? S.ch_My[(size_t)chain * D + lane + 64 * k] : 0.0;
        } else matvec(yv, My);
        double pa = 0.0;
#pragma unroll
        for (int k = 0; k < DPL; ++k) pa += yv[k] * My[k];
        C.qa = wsum<DPL, NROWS>(pa);
    }

    // ---- deck: first direction stays, the others are Fisher-Yates shuffled (chordal_sampling.f90:135-142,
    //      random_utils.F90:505-532).  deck value for position p lives in lane p when nr <= 64.
    // seq_mode: stream positions of the shuffle draws (after the seed draws and every basis) and of the slice draws
    const unsigned long long seq_g0 = seq_mode ? S.ctl->seq + 2ull + (unsigned long long)S.n_dev : 0ull;
    unsigned long long seq_run = seq_g0 + (unsigned long long)(nr - 1);
    int deck = lane;
    if (helped) { /* the helper's: taken over at the meeting point below */ }
    else if (deck_in_regs) deck = shuffle_deck_regs(seq_g0);
    else {
        for (int i = lane; i < nr; i += 64) {
            sdeck[i] = i;
            if (i >= 1) {
                const double u = seq_mode ? pc_seq_uniform(S, seq_g0 + (unsigned long long)(nr - 1 - i))
                                            : pc_uniform(S.k0, S.k1, PC_DOM_SHUFFLE, batch, (uint32_t)chain, (uint32_t)i);
                int j = (int)ceil(u * i);
                sj[i] = j < 1 ? 1 : (j > i ? i : j);
            }
        }
        __syncthreads();
        if (lane == 0)
            for (int i = nr - 1; i >= 1; --i) { const int j = sj[i], t = sdeck[i]; sdeck[i] = sdeck[j]; sdeck[j] = t; }
        __syncthreads();
    }

#if defined(SLICE_DBG) && SLICE_DBG == 2
    const long long kp3 = clock64();
#endif
    double ua = 0.0, ub = 0.0;                     // uniforms of 4 consecutive slices, 32 each
    double nh[DPL], nh_next[DPL], w_next;
    bool have_qc = false; double qc_next = 0.0; const double *qcT = nullptr;      // (LEAN = 1 with a helper: s.M.s of every direction, made with the whitening)
    // ---- FW: all directions of the chain whitened up front, lane = direction (what a thread of k_nhats did for its
    //      vector, same loops): w = L n (chordal_sampling.f90:73), |w|, n^ = w / |w|, width 3 |w| (:80-82); results in LDS
    double *nhs = nullptr, *wsh = nullptr;
    if constexpr (FW > 0) {
        double *Lsh = tbuf + (phi_lds ? (size_t)nr * (D + 1) : 0);     // [FW][D] Cholesky factor, rows past D zero
        nhs = Lsh + (size_t)FW * D;                                      // [nr][D + 1]
        wsh = nhs + (size_t)nr * (D + 1);                               // [nr]
        bool whitened = false;
        if (helped) {                                                   // the meeting point: the helper's deck, and its directions if it made them
            __syncthreads();
            deck = (lane < nr) ? sdeck[lane] : lane;
            whitened = sj[0] != 0;
            if (!whitened) preload_whitening(seed_cluster);               // (several clusters: the seed's factor was not known over there)
        } else if (seed_cluster != 0) {                                  // (uniform) several clusters: the seed's factor
            const double *Lg = S.chol + (size_t)seed_cluster * D * D;
#pragma unroll
            for (int q = 0; q < FWL; ++q) { const int e = lane + 64 * q; Lpre[q] = (e < D * D) ? Lg[e] : 0.0; }
        }
        if (!whitened) whiten_all(Lsh, nhs, wsh, nullptr, nullptr);
        const int v0 = deck_in_regs ? __builtin_amdgcn_readlane(deck, 0) : sdeck[0];
        nh_next[0] = (lane < D) ? nhs[(size_t)v0 * (D + 1) + lane] : 0.0;
        w_next = wsh[v0];
        if constexpr (LEAN == 1) { if (helped && whitened && !(S.ablate & PC_ABL_QC_BY_CHAIN)) { have_qc = true; qcT = wsh + nr + (size_t)((nr + 3) / 4) * 128; qc_next = qcT[v0]; } }
    } else
    {   // prefetch the first direction
        const int v0 = deck_in_regs ? __builtin_amdgcn_readlane(deck, 0) : sdeck[0];
        const double *p = S.nhat + ((size_t)chain * nr + v0) * D;
#pragma unroll
        for (int k = 0; k < DPL; ++k) nh_next[k] = ld.on[k] ? p[lane + 64 * k] : 0.0;
        w_next = S.nhat_w[(size_t)chain * nr + v0];
        if (msp) {
            const double *pm = S.nhat_Ms + ((size_t)chain * nr + v0) * D;
#pragma unroll
            for (int k = 0; k < DPL; ++k) Ms_next[k] = ld.on[k] ? pm[lane + 64 * k] : 0.0;
        }
    }

#ifdef SLICE_DBG
    long long scy[6] = {0, 0, 0, 0, 0, 0}; long long nev = 0, ev2 = 0;
#if SLICE_DBG == 3
    long long hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
#if SLICE_DBG == 2
    const long long kc1 = clock64();
#endif
#endif
    double w = w_next, qc_cur = qc_next;
#pragma unroll
    for (int k = 0; k < DPL; ++k) nh[k] = nh_next[k];
    // loop-invariant addresses (the per-slice address arithmetic was a third of the slice's instructions)
    const double *nh_base = S.nhat + (size_t)chain * nr * D + lane;
    const double *nw_base = S.nhat_w + (size_t)chain * nr;
    const double *nm_base = msp ? S.nhat_Ms + (size_t)chain * nr * D + lane : nh_base;
    if (msp) {
#pragma unroll
        for (int k = 0; k < DPL; ++k) Ms[k] = Ms_next[k];
    }
    double *row = S.babies + (size_t)chain * nr * nT;
    double *bl_row = S.baby_logL + (size_t)chain * nr;
    double *bl_col = S.baby_logL_T + chain;
    double *tb_row = tbuf + lane;
    const int o_p0 = S.p0, o_d0 = S.d0, o_b0 = S.b0, o_l0 = S.l0, nDer = S.nDer, Bstride = S.B;
    int nl_grade[PC_MAX_GRADE];                    // evaluations per grade (chordal_sampling.f90:84), static indices only
#pragma unroll
    for (int g = 0; g < PC_MAX_GRADE; ++g) nl_grade[g] = 0;
    for (int s = 0; s < nr; ++s, row += nT, bl_col += Bstride, tb_row += D + 1) {
#ifdef SLICE_DBG
        const long long c0 = clock64();
#endif
        const int nl_before = C.nlike;
        int my_grade = 0;
        if (graded) my_grade = pc_grade_of(S, deck_in_regs ? __builtin_amdgcn_readlane(deck, s) : sdeck[s]);
        if constexpr (FW > 0) {
            if (s + 1 < nr) {
                const int v1 = deck_in_regs ? __builtin_amdgcn_readlane(deck, s + 1) : sdeck[s + 1];
                nh_next[0] = (lane < D) ? nhs[(size_t)v1 * (D + 1) + lane] : 0.0;
                w_next = wsh[v1];
                if (LEAN == 1 && have_qc) qc_next = qcT[v1];
            }
        } else
        if (s + 1 < nr) {                           // prefetch the next direction (hidden under this slice)
            const int v1 = deck_in_regs ? __builtin_amdgcn_readlane(deck, s + 1) : sdeck[s + 1];
            const double *p = nh_base + v1 * D;
#pragma unroll
            for (int k = 0; k < DPL; ++k) nh_next[k] = ld.on[k] ? p[64 * k] : 0.0;
            w_next = nw_base[v1];
            if (msp) {
                const double *pm = nm_base + v1 * D;
#pragma unroll
                for (int k = 0; k < DPL; ++k) Ms_next[k] = ld.on[k] ? pm[64 * k] : 0.0;
            }
        }
        if ((s & 3) == 0 && !seq_mode) {          // one Philox call per lane covers 4 slices x 32 uniforms
            if (helped && s > 0) {                  // (the helper's: made while the slices before were sampled)
                const int g = s >> 2;
                while (__hip_atomic_load(&sj[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < g) __builtin_amdgcn_s_sleep(1);
                const double *U = wsh + nr;
                ua = U[((size_t)g * 64 + lane) * 2]; ub = U[((size_t)g * 64 + lane) * 2 + 1];
            } else {
            const uint32_t sl = (uint32_t)s + (uint32_t)(lane >> 4);
            pc_uniform2(S.k0, S.k1, PC_DOM_SLICE, batch, (uint32_t)chain,
                        (sl * PC_SLICE_STRIDE) / 2 + (uint32_t)(lane & 15), ua, ub);
            }
        }
        uint32_t kdraw = 0;
        auto next_u = [&]() -> double {
            if (seq_mode) return pc_seq_uniform(S, seq_run++);
            const uint32_t k = kdraw++;
            if (k < 32u) {
                const int src = ((s & 3) << 4) + (int)(k >> 1);
                return (k & 1u) ? readlane_f64(ub, src) : readlane_f64(ua, src);
            }
            return pc_uniform(S.k0, S.k1, PC_DOM_SLICE, batch, (uint32_t)chain, (uint32_t)s * PC_SLICE_STRIDE + k);
        };

#ifdef SLICE_DBG
        const long long c1 = clock64();
#endif
        double cube[DPL], th[DPL];
        if (C.quad) {
            double pa = 0.0, pb = 0.0, pc = 0.0;
            if (!corr) {
#pragma unroll
                for (int k = 0; k < DPL; ++k) {
                    const double zA = ((ld.lo[k] + ld.span[k] * x0[k]) - S.like.mu) * S.like.inv_sigma;
                    const double zB = (ld.span[k] * nh[k]) * S.like.inv_sigma;
                    if (ld.on[k]) { pa += zA * zA; pb += zA * zB; if (!(LEAN == 1 && have_qc)) pc += zB * zB; }
                }
            } else {
#pragma unroll
                for (int k = 0; k < DPL; ++k) sv[k] = ld.on[k] ? ld.span[k] * nh[k] : 0.0;
                if (!msp) matvec(sv, Ms);
#pragma unroll
                for (int k = 0; k < DPL; ++k) { pb += sv[k] * My[k]; pc += sv[k] * Ms[k]; }
            }
            // (the slice's wave sums side by side: each its own tree, a level of one between the levels of the others)
            constexpr int NR_ = DPL > 1 ? 4 : NROWS;
            if (!corr) {
                if (LEAN == 1 && have_qc) { row_sum2(pa, pb); C.qc = qc_cur; }
                else { row_sum3(pa, pb, pc); C.qc = wave_sum_rows<NR_>(pc); }
                C.qa = wave_sum_rows<NR_>(pa); C.qb = wave_sum_rows<NR_>(pb);
            } else {
                row_sum2(pb, pc);
                C.qb = wave_sum_rows<NR_>(pb); C.qc = wave_sum_rows<NR_>(pc);
            }
        }
        // initial bracket (chordal_sampling.f90:213-219)
        const double u0 = next_u();
        double tR = (1 - u0) * w, tL = -(u0 * w);
        double lR, lL;
        eval_pair<DPL, NROWS, KINDV>(C, x0, nh, tR, tL, lR, lL);
#ifdef SLICE_DBG
        const long long c2 = clock64();
#endif
        // stepping out (:223-236)
        int istepR = 0, istepL = 0;
        if (C.quad && !seq_mode) {
            // The first pc_step_spec candidates of each side at once.  Where candidate j lies -- w j to the right, -(w j) to the left -- does
            // not depend on any likelihood, and with the closed form along the chord one more candidate is a handful of operations: so they
            // are computed in straight-line code, as the shrinkage's four trials below, and each side takes the first one that ends the
            // reference's loop; the candidates behind it never happened (not counted).  A loop iteration is one dependent chain through the
            // vector unit, the scalar unit and two or three taken branches; here the state moves by selects.  A side that none of the
            // candidates ends goes on in the loop below with candidate pc_step_spec + 1 (its test fails at once for every other side).
            bool goR = (lR >= contour) & (lR > logzero), goL = (lL >= contour) & (lL > logzero);
            int cnt = 0;
#if defined(SLICE_DBG) && SLICE_DBG == 3
            int nR = 0, nL = 0;
#endif
#pragma unroll
            for (int j = 1; j <= pc_step_spec; ++j) {
                const double tr = w * j, tl = -(w * j);
                unsigned long long oR = 0ull, oL = 0ull;
#pragma unroll
                for (int k = 0; k < DPL; ++k) {
                    const double cR = x0[k] + tr * nh[k], cL = x0[k] + tl * nh[k];
                    const unsigned long long on = pc_lanes(ld.on[k]);
                    oR |= (pc_lanes(cR < 0.0) | pc_lanes(cR > 1.0)) & on; oL |= (pc_lanes(cL < 0.0) | pc_lanes(cL > 1.0)) & on;
                }
                const double gR = C.qnorm - (C.qa + tr * (2.0 * C.qb + tr * C.qc)) / 2.0;
                const double gL = C.qnorm - (C.qa + tl * (2.0 * C.qb + tl * C.qc)) / 2.0;
                const double lr = oR != 0ull ? logzero : gR, ll = oL != 0ull ? logzero : gL;     // calculate.f90:36-38
                const bool evR = goR & (lr > logzero), evL = goL & (ll > logzero);                 // ... :44, the evaluations the loop would count
                cnt += (int)evR + (int)evL;
                tR = goR ? tr : tR; lR = goR ? lr : lR;
                tL = goL ? tl : tL; lL = goL ? ll : lL;
#if defined(SLICE_DBG) && SLICE_DBG == 3
                nR += (int)goR; nL += (int)goL;
#endif
                goR = evR & (lr >= contour); goL = evL & (ll >= contour);
            }
            C.nlike += cnt;
            istepR = istepL = pc_step_spec;
#if defined(SLICE_DBG) && SLICE_DBG == 3
            if (!goR) istepR = nR;
            if (!goL) istepL = nL;
#endif
        }
#if defined(SLICE_DBG) && SLICE_DBG == 3
        const int spR = istepR, spL = istepL;
#endif
        while (lR >= contour && lR > logzero) { istepR++; tR = w * istepR; lR = eval_at<DPL, NROWS, KINDV>(C, x0, nh, tR, cube, th); }
        while (lL >= contour && lL > logzero) { istepL++; tL = -(w * istepL); lL = eval_at<DPL, NROWS, KINDV>(C, x0, nh, tL, cube, th); }
#if defined(SLICE_DBG) && SLICE_DBG == 3
        // the histogram build: iterations of the reference's loop per side (right in the low word, left in the high one) and the slices whose
        // loop went on behind the straight-line candidates
        {
            const bool fbR = istepR > spR, fbL = istepL > spL;
#pragma unroll
            for (int x = 0; x < 5; ++x) hist[x] += (long long)((istepR < 4 ? istepR : 4) == x) + ((long long)((istepL < 4 ? istepL : 4) == x) << 32);
            hist[5] += 1ll + ((long long)(istepR > 0 && istepL > 0) << 32);
            hist[6] += (long long)(fbR && !fbL) + ((long long)(fbL && !fbR) << 32);
            hist[7] += (long long)(fbR && fbL);
        }
#endif
#ifdef SLICE_DBG
        const long long c3 = clock64();
#endif
        // shrinkage (:240-271)
        double lnew = logzero, t_last = 0.0;
        bool ok = false;
        int it0 = 0;
        if (C.quad && !seq_mode) {
            // The first four trial points at once.  Where trial q lands does not depend on the likelihood of the trials
            // before it, only on their positions (a rejected trial becomes the bracket end on its side of x0), and the
            // uniforms are known: so the four positions "if everything before was rejected" are computed up front and
            // their likelihoods -- closed form along the chord -- are evaluated in straight-line code instead of a loop with a
            // divergence test per trial.  The first accepted one is the baby; the trials after it never happened (not counted,
            // their draws given back): the same result and the same likelihood count as the loop.  (Written in round 4 in the
            // belief that a dependent fp64 operation waits 32 cycles; it is the loop's branches it saves -- a wave issues every
            // 5-6 cycles, dependent or not, tools/dev/ubench_fp64.hip.  NSP = 2 measured the same within a box's noise.)
            constexpr int NSP = 4;
            const uint32_t kd0 = kdraw;
            double tc[NSP], lc[NSP], tLb[NSP], tRb[NSP];
            bool oc[NSP];
            double tLc = tL, tRc = tR;
#pragma unroll
            for (int q = 0; q < NSP; ++q) {
                const double dl = fabs(tLc), dr = fabs(tRc);
                const double t = next_u() * (dr + dl) - dl;
                tc[q] = t;
                if (t > 0.0) tRc = t; else tLc = t;
                tLb[q] = tLc; tRb[q] = tRc;                         // the bracket after rejecting trial q
                unsigned long long om = 0ull;
#pragma unroll
                for (int k = 0; k < DPL; ++k) {
                    const double cb = x0[k] + t * nh[k];
                    om |= (pc_lanes(cb < 0.0) | pc_lanes(cb > 1.0)) & pc_lanes(ld.on[k]);
                }
                oc[q] = om != 0ull;
                lc[q] = C.qnorm - (C.qa + t * (2.0 * C.qb + t * C.qc)) / 2.0;
            }
            // (a chain of ifs that leaves at the first accepted trial -- most slices accept the first or second: the same decisions as selects
            //  over all four trials measured 3 us a launch slower, with scalar branches on the lane masks level: profiles/slice_stepping.json)
            int acc = -1;
#pragma unroll
            for (int q = 0; q < NSP; ++q) {
                if (acc < 0) {
                    const double lg = oc[q] ? logzero : lc[q];     // calculate.f90:36-38
                    if (!oc[q] && lg > logzero) C.nlike++;
                    t_last = tc[q]; lnew = lg;
                    if (lg < contour || lg <= logzero) { tL = tLb[q]; tR = tRb[q]; }
                    else acc = q;
                }
            }
            if (acc >= 0) {
                ok = true; kdraw = kd0 + (uint32_t)acc + 1u;
#pragma unroll
                for (int k = 0; k < DPL; ++k) { cube[k] = x0[k] + t_last * nh[k]; th[k] = ld.lo[k] + ld.span[k] * cube[k]; }
            }
            it0 = NSP;
        }
        for (int it = it0; it <= 100 && !ok; ++it) {
            const double dl = fabs(tL), dr = fabs(tR);
            const double t = next_u() * (dr + dl) - dl;
            t_last = t;
            lnew = eval_at<DPL, NROWS, KINDV>(C, x0, nh, t, cube, th);
#ifdef SLICE_DBG
            nev++;
#endif
            if (lnew < contour || lnew <= logzero) { if (t > 0.0) tR = t; else tL = t; }
            else ok = true;
        }
        if (!ok) lnew = logzero;                    // "Non deterministic loglikelihood"
#ifdef PCHIP_USER_TERMS
        // (no point in 101 trials: the row gets the last trial's theta -- zeros if that was outside the cube --, the sum of that theta goes with it)
        if (!ok && LEAN == 0 && S.like.kind == PC_LIKE_SOURCE) (void)like_eval_terms<DPL>(S, th, ld, lane, ybuf, C.tsum);
#endif
        if (corr) {                                 // the next start point: y and M.y move along the chord
            C.qa = C.qa + t_last * (2.0 * C.qb + t_last * C.qc);
#pragma unroll
            for (int k = 0; k < DPL; ++k) { yv[k] += t_last * sv[k]; My[k] += t_last * Ms[k]; }
            if ((s & 15) == 15 && !msp) {            // resynchronise the carried products now and then
                matvec(yv, My);
                double pa = 0.0;
#pragma unroll
                for (int k = 0; k < DPL; ++k) pa += yv[k] * My[k];
                C.qa = wsum<DPL, NROWS>(pa);
            }
        }
#ifdef SLICE_DBG
        const long long c4 = clock64();
#endif
        // the baby becomes the next start point (chordal_sampling.f90:85-88)
        // The prefetched direction is taken over BEFORE this slice's stores are issued: its loads were
        // issued a whole slice ago, whereas a wait placed after the stores (vmcnt counts them too on
        // gfx9) would stall every slice for a full store round trip.
        w = w_next; qc_cur = qc_next;
#pragma unroll
        for (int k = 0; k < DPL; ++k) { nh[k] = nh_next[k]; asm volatile("" : "+v"(nh[k])); }
        asm volatile("" : "+v"(w));
        if (msp) {
#pragma unroll
            for (int k = 0; k < DPL; ++k) { Ms[k] = Ms_next[k]; asm volatile("" : "+v"(Ms[k])); }
        }
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            x0[k] = cube[k];
            // (written THROUGH the L2 -- system scope -- so that the launch does not end on the write-back of a nursery's 8 MB of rows, which the
            //  contraction behind it waited for: 11.61 -> 11.49 ms a run, three A/B pairs on one box)
            if (ld.on[k]) { __hip_atomic_store(&row[lane + 64 * k], cube[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); __hip_atomic_store(&row[o_p0 + lane + 64 * k], th[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
        }
        if (phi_lds) {
#pragma unroll
            for (int k = 0; k < DPL; ++k) if (ld.on[k]) tb_row[64 * k] = th[k];
#ifdef PCHIP_USER_TERMS
#ifdef PCHIP_USER_SUMS
            if (LEAN == 0 && lane == 0 && S.like.kind == PC_LIKE_SOURCE) {
#pragma unroll
                for (int k = 0; k < PC_NSUMS; ++k) sums_lds[(size_t)s * PC_NSUMS + k] = C.tsum[k];
            }
#else
            if (LEAN == 0 && lane == 0) tb_row[D] = C.tsum[0];     // (lane 0: tb_row is the row's start)
#endif
#endif
        } else if (!lean2 && nDer > 0) {
#ifdef PCHIP_USER_TERMS
            if (LEAN == 0 && S.like.kind == PC_LIKE_SOURCE) like_phi_terms<DPL>(S, th, ld, lane, ybuf, C.tsum, row + o_d0); else
#elif defined(PCHIP_USER_SOURCE)
            if (LEAN == 0 && S.like.kind == PC_LIKE_SOURCE) like_phi_source<DPL>(S, th, ld, lane, ybuf, row + o_d0); else
#endif
            {
            double phi0, phi1;
            like_phi<DPL, NROWS, KINDV>(S, th, ld, lane, phi0, phi1);
            if (lane == 0) {
                row[o_d0] = phi0;
                if (nDer >= 2) row[o_d0 + 1] = phi1;
                for (int e = 2; e < nDer; ++e) row[o_d0 + e] = 0.0;
            }
            }
        }
        if (lane == 0) {
            row[o_b0] = contour;                    // nested_sampling.F90:260
            row[o_l0] = lnew;
            bl_row[s] = lnew; *bl_col = lnew;
        }
        if (graded) {
#pragma unroll
            for (int g = 0; g < PC_MAX_GRADE; ++g) nl_grade[g] += (my_grade == g) ? C.nlike - nl_before : 0;
        }
#ifdef SLICE_DBG
        const long long c5 = clock64();
        scy[0] += c1 - c0; scy[1] += c2 - c1; scy[2] += c3 - c2; scy[3] += c4 - c3; scy[4] += c5 - c4;
#endif
    }
#if defined(SLICE_DBG) && SLICE_DBG == 2
    const long long kc2 = clock64();
#elif defined(SLICE_DBG) && SLICE_DBG == 3
    if (lane == 0) for (int x = 0; x < 8; ++x) atomicAdd((unsigned long long *)&S.ctl->dbg[x], (unsigned long long)hist[x]);      // (every chain)
#elif defined(SLICE_DBG)
    if (lane == 0 && chain == 0) { for (int x = 0; x < 5; ++x) S.ctl->dbg[x] += scy[x]; S.ctl->dbg[5] += nev; S.ctl->dbg[6] += scy[5]; S.ctl->dbg[7] += ev2; }
#endif
    if (lane == 0) S.ch_nlike[chain] = C.nlike;
    if (graded) {
        if (lane == 0) {
#pragma unroll
            for (int g = 0; g < PC_MAX_GRADE; ++g) S.ch_nlike_g[(size_t)chain * PC_MAX_GRADE + g] = nl_grade[g];
        }
    }
    if (seq_mode && lane == 0 && chain == 0) S.ctl->seq = seq_run;
    // derived parameters of all the babies at once, lane = slice (gaussian.f90:36-37, twin_gaussian.f90:48-52):
    // one sqrt / log per chain instead of one per slice on the chain's critical path
    if (!lean2 && S.nDer > 0 && phi_lds) {
        __syncthreads();                            // one wave per workgroup: orders the LDS writes above
        for (int s0 = 0; s0 < nr; s0 += 64) {
            const int s = s0 + lane;
            if (s >= nr) continue;
            double *row = S.babies + ((size_t)chain * nr + s) * nT;
            const double *tt = tbuf + (size_t)s * (D + 1);
#ifdef PCHIP_USER_SHARED
            // (shared values: finish needs the point's shared block, and a lane = baby has none -- pc_slice_phi_lds never sets phi_lds for such a
            //  handle, its derived parameters are written inside the slice loop, and no branch of the source is compiled here)
#elif defined(PCHIP_USER_TERMS)
            if (LEAN == 0 && S.like.kind == PC_LIKE_SOURCE) {   // finish(sums, theta) of the baby's kept sums, lane = baby: no walk over the data
                double phi[PC_SRC_MAX_DERIVED];
#ifdef PCHIP_USER_SUMS
                (void)pc_user_finish(sums_lds + (size_t)s * PC_NSUMS, tt, phi, D, S.nDer, S.src_data, (long)S.src_ndata);
#else
                (void)pc_user_finish(tt + D, tt, phi, D, S.nDer, S.src_data, (long)S.src_ndata);
#endif
                for (int e = 0; e < S.nDer; ++e) row[S.d0 + e] = phi[e];
                continue;
            }
#elif defined(PCHIP_USER_SOURCE)
            if (LEAN == 0 && S.like.kind == PC_LIKE_SOURCE) {   // the user's function, lane = baby
                double phi[PC_SRC_MAX_DERIVED];
                (void)pchip_loglikelihood(tt, phi, D, S.nDer, S.src_data, (long)S.src_ndata);
                for (int e = 0; e < S.nDer; ++e) row[S.d0 + e] = phi[e];
                continue;
            }
#endif
            double phi0 = 0.0, phi1 = 0.0;
            if (lean || LEAN == 5 || (LEAN == 0 && S.like.kind == PC_LIKE_GAUSSIAN)) {
                double r2 = 0.0;
                for (int d = 0; d < D; ++d) { const double z = tt[d] - S.like.mu; r2 += z * z; }
                phi0 = sqrt(r2);
                if (S.nDer >= 2) phi1 = pc_log_ball(phi0, D, S.like.log_vn);
            } else if (LEAN == 4 || (LEAN == 0 && S.like.kind == PC_LIKE_TWIN_GAUSSIAN)) {
                phi0 = (tt[0] > 0.5) ? 1.0 : -1.0;
            }
            row[S.d0] = phi0;
            if (S.nDer >= 2) row[S.d0 + 1] = phi1;
            for (int e = 2; e < S.nDer; ++e) row[S.d0 + e] = 0.0;
        }
    }
#if defined(SLICE_DBG) && SLICE_DBG == 2
    // whole-kernel view, all chains: cycles before / inside / after the slice loop (sums and maxima), launch-relative start
    {
        const long long kc3 = clock64(), kw3 = wall_clock64();
        unsigned long long *g = (unsigned long long *)S.ctl->dbg;
        if (lane == 0) {
            atomicAdd(&g[0], (unsigned long long)(kp1 - kc0)); atomicAdd(&g[1], (unsigned long long)(kp2 - kp1)); atomicAdd(&g[2], (unsigned long long)(kp3 - kp2));
            atomicAdd(&g[3], (unsigned long long)(kc1 - kp3)); atomicAdd(&g[4], (unsigned long long)(kc2 - kc1)); atomicAdd(&g[5], (unsigned long long)(kc3 - kc2));
            atomicMax(&g[6], (unsigned long long)(kw3 - kw0));       // longest chain, 100 MHz ticks
        }
    }
#endif
