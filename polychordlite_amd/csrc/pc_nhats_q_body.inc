// pc_nhats_q_body.inc -- the body of k_nhats_q (pc_bases.hip), included by the one-run kernel and by k_nhats_q_many (several runs in
// step, blockIdx.z = run): the same statements on `S` and `batch`.  Not a header: no include guard.
    constexpr int DP = 4 * HV, NTQ = 16 * HV;
    // LDS rows are stored as four coordinate blocks of HV + 2 doubles: the four threads of a vector read their blocks
    // at the same time, and blocks exactly HV doubles (a multiple of 256 B) apart would all start in the same bank
    constexpr int HP = HV + 2, DPP = 4 * HP;
    extern __shared__ __attribute__((aligned(16))) char smem_q[];
    double (*Qb)[DPP] = (double (*)[DPP])smem_q;                      // [2][DPP] pivot, double buffered
    double (*Lt)[DPP] = (double (*)[DPP])(smem_q + sizeof(double) * 2 * DPP);   // [HV][DPP] HV rows of the Cholesky factor (HV < 32)
    __shared__ int sh[2];
    const int D = S.D, nr = S.nr;
    const int tid = threadIdx.x, chain = blockIdx.y;
    const int i = tid >> 2, h = tid & 3, d0 = HV * h, p0 = HP * h;    // my vector, my coordinate block (p0: in LDS rows)
    int grade, basis;                                                 // chordal_sampling.f90:119-130, see k_nhats
    pc_grade_of_basis(S, blockIdx.x, grade, basis);
    const int off = pc_sel(S.g_off, grade), Dg = D - off, nrg = pc_sel(S.g_nr, grade), col0 = pc_sel(S.g_col0, grade);
    const bool active = i < Dg;
#ifdef NHATSQ_DBG
    long long qc[6]; qc[0] = clock64();
#endif
    if (PART != 1 && tid == 0) {
        int sel, slot;
        select_seed(S, batch, chain, sel, slot);
        sh[0] = sel; sh[1] = slot;
        if (blockIdx.x == 0) {
            S.ch_cluster[chain] = sel; S.ch_seed_slot[chain] = slot;
            S.ch_contour[chain] = S.logLp[sel];          // nested_sampling.F90:270
            S.ch_epoch[chain] = S.ctl->admin_epoch;
            if (chain == 0) { S.ctl->i_nursery = gridDim.y; S.ctl->batch_id = batch; }
        }
    }
    double *rawb = (PART != 0) ? S.nhat_raw + ((size_t)chain * S.nb_total + blockIdx.x) * (size_t)(HV * NTQ) : nullptr;
    // gaussian deviates of my 32 coordinates: element (basis*D + i)*D + d of stream (batch, chain) in PC_DOM_NHAT,
    // two per Philox call
    double v[HV];
#pragma unroll
    for (int e = 0; e < HV; ++e) v[e] = 0.0;
    double lpre[(HV * DP + NTQ - 1) / NTQ];
    if constexpr (PART == 2 && HV < 32) {
        // second half (nDims 25 ... 64, one grade): the orthonormal basis was made by part 1 -- drawn on the side stream under an earlier
        // nursery's contraction, it depends on the keys and the nursery's number only -- and lies in nhat_raw thread by thread
#pragma unroll
        for (int e = 0; e < HV; ++e) v[e] = rawb[(size_t)tid * HV + e];
        __syncthreads();                                               // (sh[]: the seed's cluster)
        const double *Lc0 = S.chol + (size_t)sh[0] * D * D;
#pragma unroll
        for (int x = 0; x < (HV * DP + NTQ - 1) / NTQ; ++x) {
            const int y = tid + x * NTQ, r = y / DP, b = y % DP;
            lpre[x] = (y < HV * DP && r < D && b < D) ? Lc0[(size_t)r * D + b] : 0.0;
        }
    } else {
    if (active) {
        // stream element of my register 0 (coordinate d0); registers [r_lo, r_hi) hold coordinates that exist and move
        const long long e0 = (long long)(S.seq_mode ? (uint32_t)S.ctl->seq + 2u : 0u) + pc_sel(S.g_e0, grade)
                             + ((long long)basis * Dg + i) * Dg + (d0 - off);
        const int r_lo = max(0, off - d0), r_hi = min(HV, D - d0);
        if (r_hi > r_lo) {
            // Philox call number cbase + cc holds stream elements 2 (cbase + cc) and + 1, i.e. my registers 2 cc - par and
            // 2 cc - par + 1 with par = parity of e0: every call lands in one of two fixed register pairs
            const long long cbase = e0 >> 1;
            const bool par = (e0 & 1ll) != 0;
#pragma unroll
            for (int cc = 0; cc < HV / 2 + 1; ++cc) {
                const int ea = 2 * cc - (par ? 1 : 0), eb = ea + 1;
                if (eb >= r_lo && ea < r_hi) {
                    const uint32_t call = (uint32_t)(cbase + cc);
                    double ua, ub;
                    if (S.seq_mode) pc_uniform2(S.k0, S.k1, PC_DOM_SEQ, 0u, 0u, call, ua, ub);
                    else pc_uniform2(S.k0, S.k1, PC_DOM_NHAT, batch, (uint32_t)chain, call, ua, ub);
                    const double ga = pc_inv_normal_cdf(ua), gb = pc_inv_normal_cdf(ub);
                    if (2 * cc - 1 >= 0 && 2 * cc - 1 < HV) v[(2 * cc - 1 >= 0 && 2 * cc - 1 < HV) ? 2 * cc - 1 : 0] = par ? ga : v[(2 * cc - 1 >= 0 && 2 * cc - 1 < HV) ? 2 * cc - 1 : 0];
                    if (2 * cc < HV) v[2 * cc < HV ? 2 * cc : 0] = par ? gb : ga;
                    if (2 * cc + 1 < HV) v[2 * cc + 1 < HV ? 2 * cc + 1 : 0] = par ? v[2 * cc + 1 < HV ? 2 * cc + 1 : 0] : gb;
                }
            }
#pragma unroll
            for (int e = 0; e < HV; ++e) v[e] = (e >= r_lo && e < r_hi) ? v[e] : 0.0;   // coordinates that do not exist / do not move
        }
    }
#ifdef NHATSQ_DBG
    qc[1] = clock64();
#endif
#define PC_DOT32(RES, A, B) { double p0_ = 0.0, p1_ = 0.0, p2_ = 0.0, p3_ = 0.0; \
        _Pragma("unroll") for (int e = 0; e < HV; e += 4) { \
            p0_ += (A)[e] * (B)[e]; p1_ += (A)[e + 1] * (B)[e + 1]; p2_ += (A)[e + 2] * (B)[e + 2]; p3_ += (A)[e + 3] * (B)[e + 3]; } \
        RES = quad_sum((p0_ + p1_) + (p2_ + p3_)); }
    {   // random_direction (random_utils.F90:276-298)
        double n2;
        PC_DOT32(n2, v, v)
        const double inrm = active ? 1.0 / sqrt(n2) : 0.0;
#pragma unroll
        for (int e = 0; e < HV; ++e) v[e] *= inrm;
    }
    if (i == 0) {
#pragma unroll
        for (int e = 0; e < HV; ++e) Qb[0][p0 + e] = v[e];
    }
    __syncthreads();
    // first tile of the Cholesky factor: requested now, consumed after the loop
    if constexpr (HV < 32 && PART != 1) {
        const double *Lc0 = S.chol + (size_t)sh[0] * D * D;
#pragma unroll
        for (int x = 0; x < (HV * DP + NTQ - 1) / NTQ; ++x) {
            const int y = tid + x * NTQ, r = y / DP, b = y % DP;
            lpre[x] = (y < HV * DP && r < D && b < D) ? Lc0[(size_t)r * D + b] : 0.0;
        }
    }
#ifdef NHATSQ_DBG
    qc[2] = clock64();
#endif
    // Gram-Schmidt (random_utils.F90:391-399): same projections as before, pivot unnormalised
    for (int j = 0; j < Dg; ++j) {
        // a wave whose sixteen vectors are all finished (i < j) only keeps the barrier company
        if ((((tid >> 6) + 1) << 4) <= j) { __syncthreads(); continue; }
        double q[HV];
#pragma unroll
        for (int e = 0; e < HV; ++e) q[e] = Qb[j & 1][p0 + e];
        double qq, dv;
        PC_DOT32(qq, q, q)
        PC_DOT32(dv, q, v)
        if (i == j) {
            const double inrm = 1.0 / sqrt(qq);
#pragma unroll
            for (int e = 0; e < HV; ++e) v[e] *= inrm;
        } else if (active && i > j) {
            const double cproj = dv / qq;
#pragma unroll
            for (int e = 0; e < HV; ++e) v[e] -= cproj * q[e];
            if (i == j + 1) {
#pragma unroll
                for (int e = 0; e < HV; ++e) Qb[(j + 1) & 1][p0 + e] = v[e];
            }
        }
        __syncthreads();
    }
#ifdef NHATSQ_DBG
    qc[3] = clock64();
#endif
    }
    if constexpr (PART == 1 && HV < 32) {
#pragma unroll
        for (int e = 0; e < HV; ++e) rawb[(size_t)tid * HV + e] = v[e];  // (thread by thread: part 2 is this kernel again)
        return;
    }
    if constexpr (PART == 1) {
        // the layout k_whiten reads as its B operand: [n][group of sixteen vectors][lk][vector in group], coordinate
        // 32 h + e = 8 (n >> 1) + 2 lk + (n & 1)
#pragma unroll
        for (int e = 0; e < HV; ++e) {
            const int n = 8 * h + 2 * (e >> 3) + (e & 1), lkk = (e & 7) >> 1;
            rawb[((size_t)n * 8 + (i >> 4)) * 64 + lkk * 16 + (i & 15)] = v[e];
        }
        return;
    }
    // whitening  w = L.n  (chordal_sampling.f90:73): tile k holds rows 32k..32k+31 of L, i.e. exactly the output
    // coordinates of block h = k
    const int col = col0 + basis * Dg + i;
    const bool wanted = basis * Dg + i < nrg;
    const double *Lc = S.chol + (size_t)sh[0] * D * D;
    if constexpr (HV == 32) {
        // nDims 65..128: W = L.N on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  The basis goes to LDS (row = vector,
        // odd row stride), L passes through LDS sixteen rows at a time (lower triangle only), wave tj owns the sixteen
        // output columns (vectors) 16 tj ..: it keeps their tiles in registers, normalises, and writes whole rows.
        // Operand maps as in k_cov_partial: A[i=lane&15][k=lane>>4], B[k=lane>>4][j=lane&15], D row = (lane>>4)+4 reg.
        typedef double v4d __attribute__((ext_vector_type(4)));
        constexpr int NS = 129;
        const int nt = (D + 15) >> 4, NR = nt * 16;
        double *Nl = (double *)smem_q + 2 * DPP;                       // [NR][NS]
        double *L16 = Nl + (size_t)NR * NS;                            // [2][16][NS]: the tile in use and the next one
        const bool dbuf = NR <= 112;                                   // (beyond: one buffer, and a barrier before it is refilled)
        // tiles of L (and of M below) travel global -> registers -> LDS one tile ahead of the matrix cores: one barrier per tile
        double pre[4];
        auto load_L = [&](int ti) __attribute__((always_inline)) {
            const int kmax = min(NR, 16 * (ti + 1));                   // L(a, b) = 0 for b > a
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int x = tid + q * NTQ, r = x / kmax, bcol = x - r * kmax, arow = 16 * ti + r;
                pre[q] = (x < 16 * kmax && arow < D && bcol < D) ? Lc[(size_t)arow * D + bcol] : 0.0;
            }
        };
        auto store_L = [&](int ti) __attribute__((always_inline)) {
            const int kmax = min(NR, 16 * (ti + 1));
            double *buf = L16 + (size_t)(dbuf ? (ti & 1) : 0) * 16 * NS;
            if (!dbuf) __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int x = tid + q * NTQ, r = x / kmax, bcol = x - r * kmax;
                if (x < 16 * kmax) buf[(size_t)r * NS + bcol] = pre[q];
            }
        };
        load_L(0);
        if (i < NR) {
#pragma unroll
            for (int e = 0; e < HV; ++e) Nl[(size_t)i * NS + d0 + e] = v[e];    // zero beyond nDims and beyond the basis
        }
        const int lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
        v4d acc[8];
#pragma unroll
        for (int ti = 0; ti < 8; ++ti) acc[ti] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ti = 0; ti < 8; ++ti) {
            if (ti < nt) {
                store_L(ti);
                if (ti + 1 < nt) load_L(ti + 1);
                __syncthreads();                                       // tile ti (and, the first time, the basis) complete
                if (wv < nt) {
                    const int kmax = min(NR, 16 * (ti + 1));
                    const double *pa = L16 + (size_t)(dbuf ? (ti & 1) : 0) * 16 * NS + (size_t)li * NS + lk;
                    const double *pb = Nl + (size_t)(16 * wv + li) * NS + lk;
                    v4d a4 = v4d{0.0, 0.0, 0.0, 0.0};
                    for (int k0 = 0; k0 < kmax; k0 += 4) a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0], a4, 0, 0, 0);
                    acc[ti] = a4;
                }
            }
        }
        if (wv < nt) {
            // |w| of my column (chordal_sampling.f90:80-82): my four row groups, then the other three lane groups
            double n2 = 0.0;
#pragma unroll
            for (int ti = 0; ti < 8; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) n2 += acc[ti][r] * acc[ti][r];
            n2 += __shfl_xor(n2, 16); n2 += __shfl_xor(n2, 32);
            const double wn = sqrt(n2), iw = 1.0 / wn;
            const int ivec = 16 * wv + li;                             // vector of this basis = column
            double *mine = Nl + (size_t)ivec * NS;                     // the basis rows of this wave are no longer read
#pragma unroll
            for (int ti = 0; ti < 8; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) if (ti < nt) mine[16 * ti + lk + 4 * r] = acc[ti][r] * iw;
            if (lk == 0 && ivec < Dg && basis * Dg + ivec < nrg) S.nhat_w[(size_t)chain * nr + col0 + basis * Dg + ivec] = wn * 3.0;
            // rows leave coalesced
            for (int cc = 0; cc < 16; ++cc) {
                const int iv = 16 * wv + cc;
                if (iv < Dg && basis * Dg + iv < nrg) {
                    double *out = S.nhat + ((size_t)chain * nr + col0 + basis * Dg + iv) * D;
                    const double *src = Nl + (size_t)iv * NS;
                    for (int a2 = lane; a2 < D; a2 += 64) out[a2] = src[a2];
                }
            }
        }
        if (S.nhat_Ms != nullptr) {
            // correlated Gaussian (random_gaussian.f90:17-30): along a chord the exponent is quadratic (see ChainCtx) and all a
            // slice needs of the matrix is M.s, s = span o n^.  Every direction of the chain is known HERE: the products are
            // one more [D x D] x [D x 16] pass per wave on the matrix cores (rows of M streamed through the tile buffer of L)
            // instead of a matrix-vector product per slice inside the chain.  Wave 0 of the chain's first basis also forms
            // M.(theta_seed - mean), the one product the chain needs for its start point.
            double *spn = (double *)smem_q, *y0s = spn + 128;           // the pivot buffers are free now (2 x 136 doubles)
            const double *Mt = S.like.invcov;                           // Mt[b * D + a] = M(a, b)
            auto load_M = [&](int ti) __attribute__((always_inline)) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int x = tid + q * NTQ, r = x & 15, bcol = x >> 4, arow = 16 * ti + r;
                    pre[q] = (x < 16 * NR && arow < D && bcol < D) ? Mt[(size_t)bcol * D + arow] : 0.0;
                }
            };
            auto store_M = [&](int ti) __attribute__((always_inline)) {
                double *buf = L16 + (size_t)(dbuf ? (ti & 1) : 0) * 16 * NS;
                if (!dbuf) __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int x = tid + q * NTQ, r = x & 15, bcol = x >> 4;
                    if (x < 16 * NR) buf[(size_t)r * NS + bcol] = pre[q];
                }
            };
            __syncthreads();
            if (tid < NR) {
                const bool on = tid < D;
                const double lo = (on && S.prior.lo) ? S.prior.lo[tid] : 0.0, hi = (on && S.prior.hi) ? S.prior.hi[tid] : 1.0;
                spn[tid] = on ? hi - lo : 0.0;
                const double c0 = on ? S.live[(size_t)sh[1] * S.nT + tid] : 0.0;
                y0s[tid] = on ? (lo + (hi - lo) * c0) - (S.like.mean ? S.like.mean[tid] : 0.0) : 0.0;
            }
            load_M(0);
            __syncthreads();
            if (wv < nt) {                                              // my sixteen rows: n^ -> s
                for (int x = lane; x < 16 * NR; x += 64) { const int r = x / NR, a2 = x % NR; Nl[(size_t)(16 * wv + r) * NS + a2] *= spn[a2]; }
            }
            v4d ac2[8];
#pragma unroll
            for (int ti = 0; ti < 8; ++ti) ac2[ti] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ti = 0; ti < 8; ++ti) {
                if (ti < nt) {
                    store_M(ti);
                    if (ti + 1 < nt) load_M(ti + 1);
                    __syncthreads();
                    const double *tile = L16 + (size_t)(dbuf ? (ti & 1) : 0) * 16 * NS;
                    if (wv < nt) {
                        const double *pa = tile + (size_t)li * NS + lk;
                        const double *pb = Nl + (size_t)(16 * wv + li) * NS + lk;
                        v4d a4 = v4d{0.0, 0.0, 0.0, 0.0};
                        for (int k0 = 0; k0 < NR; k0 += 4) a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0], a4, 0, 0, 0);
                        ac2[ti] = a4;
                    }
                    if (wv == 7 && blockIdx.x == 0) {                  // M.y0, rows of this tile: lane = (row, quarter of the columns)
                        double t = 0.0;
                        for (int b = lk; b < NR; b += 4) t += tile[(size_t)li * NS + b] * y0s[b];
                        t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
                        if (lk == 0 && 16 * ti + li < D) S.ch_My[(size_t)chain * D + 16 * ti + li] = t;
                    }
                }
            }
            if (wv < nt) {
                double *mine = Nl + (size_t)(16 * wv + li) * NS;
#pragma unroll
                for (int ti = 0; ti < 8; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (ti < nt) mine[16 * ti + lk + 4 * r] = ac2[ti][r];
                for (int cc = 0; cc < 16; ++cc) {
                    const int iv = 16 * wv + cc;
                    if (iv < Dg && basis * Dg + iv < nrg) {
                        double *out = S.nhat_Ms + ((size_t)chain * nr + col0 + basis * Dg + iv) * D;
                        const double *src = Nl + (size_t)iv * NS;
                        for (int a2 = lane; a2 < D; a2 += 64) out[a2] = src[a2];
                    }
                }
            }
        }
        return;
    }
    double w[HV];
#pragma unroll
    for (int e = 0; e < HV; ++e) w[e] = 0.0;
    for (int k = 0; k * HV < D; ++k) {
        __syncthreads();
        if (k == 0) {
            // the first tile was requested before the Gram-Schmidt loop (registers lpre): its latency is hidden
#pragma unroll
            for (int x = 0; x < (HV * DP + NTQ - 1) / NTQ; ++x) { const int y = tid + x * NTQ, b = y % DP; if (y < HV * DP) Lt[y / DP][(b / HV) * HP + b % HV] = lpre[x]; }
        } else {
            for (int x = tid; x < HV * DP; x += NTQ) {
                const int r = x / DP, b = x % DP, a = HV * k + r;
                Lt[r][(b / HV) * HP + b % HV] = (a < D && b < D) ? Lc[(size_t)a * D + b] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < HV; ++r) {
            double t;
            PC_DOT32(t, (&Lt[r][p0]), v)
            if (h == k) w[r] = t;
        }
    }
    if (active && wanted) {
        double n2;
        PC_DOT32(n2, w, w)
        const double wn = sqrt(n2), iw = 1.0 / wn;              // chordal_sampling.f90:80-82
        double *out = S.nhat + ((size_t)chain * nr + col) * D + d0;
#pragma unroll
        for (int e = 0; e < HV; ++e) if (d0 + e < D) out[e] = w[e] * iw;
        if (h == 0) S.nhat_w[(size_t)chain * nr + col] = wn * 3.0;
    }
#undef PC_DOT32
#ifdef NHATSQ_DBG
    qc[4] = clock64();
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) for (int x = 0; x < 4; ++x) S.ctl->gen_cyc[x] += qc[x + 1] - qc[x];
#endif
