// pc_update_steps.hip -- the "update" step taken kernel by kernel (PC_UPDATE_STEPS of pc_plan.h): any number of clusters, any nDims.
//
//   k_clean_* / k_cov_* / k_chol   clean_phantoms (run_time_info.f90:820-877) as a threshold test + deterministic stream
//               compaction, calculate_covmats (:601-641) as a two-pass mean / centred SYRK with fixed-order reduction,
//               calc_cholesky (utils.F90:621-649).
//   k_post_max, k_post_moments   the posterior moments of the dead points: here because they take the covariance kernels' thread layout (cov_dpc).
// pc_update.hip is the same update in one pass for one cluster; it launches k_scan_blocks and the Cholesky kernels of this file.
#include "pc_state.h"
#include "pc_launch.h"
#include "pc_block.h"
#include <cstdlib>

// ------------------------------------------------------------------------------------------
// update step 1: clean_phantoms (run_time_info.f90:820-877)
// A phantom of cluster c is dropped iff some death of c since the last clean has a larger logL,
// i.e. iff its logL < the logL of c's latest death; phantoms of dead clusters are dropped too.
// Deterministic 3-kernel stream compaction into the alternate phantom buffer.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int cluster_of_uid(const PcState &S, unsigned uid, int nc)
{
    for (int c = 0; c < nc; ++c) if (S.cl_uid[c] == uid) return c;
    return -1;
}

__device__ __forceinline__ void clean_flag_body(const PcState &S, int nph, unsigned char *keep, int *blk_count)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int nc = S.ctl->ncluster;
    bool k = false;
    if (j < nph) {
        const int c = cluster_of_uid(S, S.ph_cuid[j], nc);
        k = (c >= 0) && !(S.ph_logL[j] < S.death_thr[c]);
        keep[j] = k ? 1 : 0;
    }
    const unsigned long long m = __ballot(k);
    __shared__ int cnt[4];
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blk_count[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}
__global__ __launch_bounds__(256) void k_clean_flag(PcState S, int nph, unsigned char *keep, int *blk_count) { clean_flag_body(S, nph, keep, blk_count); }
__global__ __launch_bounds__(256) void k_clean_flag_many(const PcManyRec *R) { const PcManyView r = pc_many_view(R, blockIdx.y); if ((int)blockIdx.x >= r.ia[PC_REC_I_BLOCKS]) return; clean_flag_body(r.S, r.ia[PC_REC_I_ROWS], (unsigned char *)r.p[PC_REC_KEEP], (int *)r.p[PC_REC_BLK]); }


__device__ __forceinline__ void scan_blocks_body(int *blk_count, int nblk, int *total, int *total2)
{   // exclusive scan, single workgroup, fixed order
    __shared__ int carry;
    __shared__ int tmp[256];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < nblk ? blk_count[i] : 0;
        tmp[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int t = threadIdx.x >= off ? tmp[threadIdx.x - off] : 0;
            __syncthreads();
            tmp[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nblk) blk_count[i] = carry + tmp[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += tmp[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) { *total = carry; if (total2) *total2 = carry; }   // total2: the control block's phantom count
}
__global__ __launch_bounds__(256) void k_scan_blocks(int *blk_count, int nblk, int *total, int *total2) { scan_blocks_body(blk_count, nblk, total, total2); }
__global__ __launch_bounds__(256) void k_scan_blocks_many(const PcManyRec *R) { const PcManyView r = pc_many_view(R, blockIdx.y); scan_blocks_body((int *)r.p[PC_REC_BLK], r.ia[PC_REC_I_BLOCKS], (int *)r.p[PC_REC_TOTAL], &r.S.ctl->nphantom); }


__device__ __forceinline__ void clean_scatter_body(const PcState &S, int nph, const unsigned char *keep, const int *blk_off,
                                                   double *ph2, double *phL2, unsigned *phC2, unsigned long long *phU2,
                                                   int *dst_index /* [nph] or nullptr */)
{
    const int j = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const bool k = (j < nph) && keep[j];
    const unsigned long long m = __ballot(k);
    __shared__ int wcnt[4];
    if (lane == 0) wcnt[wid] = __popcll(m);
    __syncthreads();
    int woff = blk_off[blockIdx.x];
    for (int i = 0; i < wid; ++i) woff += wcnt[i];
    const int off = woff + __popcll(m & ((1ull << lane) - 1ull));
    if (dst_index && j < nph) dst_index[j] = k ? off : -1;
    if (k) { phL2[off] = S.ph_logL[j]; phC2[off] = S.ph_cuid[j]; phU2[off] = S.ph_uid[j]; }
    // rows: the wave copies its surviving rows cooperatively (coalesced, eight rows in flight)
    const int j0 = blockIdx.x * 256 + wid * 64;
    wave_copy_masked(S.phantom + (size_t)j0 * S.nT, m, ph2 + (size_t)woff * S.nT, S.nT, lane);
}
__global__ __launch_bounds__(256) void k_clean_scatter(PcState S, int nph, const unsigned char *keep, const int *blk_off,
                                                      double *ph2, double *phL2, unsigned *phC2, unsigned long long *phU2, int *dst_index)
{ clean_scatter_body(S, nph, keep, blk_off, ph2, phL2, phC2, phU2, dst_index); }
__global__ __launch_bounds__(256) void k_clean_scatter_many(const PcManyRec *R)
{
    const PcManyView r = pc_many_view(R, blockIdx.y);
    if ((int)blockIdx.x >= r.ia[PC_REC_I_BLOCKS]) return;
    clean_scatter_body(r.S, r.ia[PC_REC_I_ROWS], (const unsigned char *)r.p[PC_REC_KEEP], (const int *)r.p[PC_REC_BLK], (double *)r.p[PC_REC_PH2], (double *)r.p[PC_REC_PHL2], (unsigned *)r.p[PC_REC_PHC2], (unsigned long long *)r.p[PC_REC_PHU2], nullptr);
}


__global__ void k_reset_thresholds(PcState S) { for (int c = threadIdx.x; c < S.maxc; c += blockDim.x) S.death_thr[c] = -PC_HUGE; }
__global__ void k_reset_thresholds_many(const PcManyRec *__restrict__ R) { const PcState S = pc_many_state(R, blockIdx.y); for (int c = threadIdx.x; c < S.maxc; c += blockDim.x) S.death_thr[c] = -PC_HUGE; }

// ------------------------------------------------------------------------------------------
// update step 2: calculate_covmats (run_time_info.f90:601-641), two passes, fixed-order sums
// pass A: per (chunk, cluster) partial sums of cube coordinates; pass B: centred outer products
// rows = live slots followed by phantoms.  partial buffers: [nchunk][nc][D] and [nchunk][nc][D*D]
// ------------------------------------------------------------------------------------------
#define PC_COV_ROWS 256          /* rows per chunk */

__device__ __forceinline__ const double *cov_row(const PcState &S, int r, int nlive_slots, int nc, int &c)
{
    if (r < nlive_slots) { c = S.live_cluster[r]; return S.live + (size_t)r * S.nT; }
    const int j = r - nlive_slots;
    c = cluster_of_uid(S, S.ph_cuid[j], nc);
    return S.phantom + (size_t)j * S.nT;
}

__device__ __forceinline__ const double *cov_ptr(const PcState &S, int r)
{
    return (r < S.Ncap) ? S.live + (size_t)r * S.nT : S.phantom + (size_t)(r - S.Ncap) * S.nT;
}

// thread layout of the reductions below: DPc = coordinates handled side by side, G = 256 / DPc row groups
__device__ __forceinline__ int cov_dpc(int D) { int p = 32; while (p < D && p < 256) p <<= 1; return p; }

// s += AT at kk = k0, k0 + G, ... below n, added in that order: eight independent loads in flight at a time.  The fixed-order sum of the partials
// in k_cov_partial's mean, k_fold_partials and k_cov_final_chol.  Text, not a function, as PC_DECK_SHUFFLE of pc_seed.h is: inlined from a
// __forceinline__ function taking the element as a lambda, all three kernels' instructions change (tools/dev/isa_diff.py).
#define PC_STRIDED_SUM(s, k0, n, G, kk, AT) { \
    int k_ = (k0); \
    for (; k_ + 7 * (G) < (n); k_ += 8 * (G)) { \
        double t8[8]; \
        _Pragma("unroll") \
        for (int u = 0; u < 8; ++u) { const int kk = k_ + u * (G); t8[u] = AT; } \
        _Pragma("unroll") \
        for (int u = 0; u < 8; ++u) s += t8[u]; \
    } \
    for (; k_ < (n); k_ += (G)) { const int kk = k_; s += AT; } }

__global__ __launch_bounds__(256) void k_cov_mean_partial(PcState S, int nrows, int nph, double *psum, int *pcnt, int CR)
{
    // grid (nchunk, nc); thread = (row group g, coordinate d): group g sums rows r0+g, r0+g+G, ... of
    // cluster c in that order, the groups are added in order: a fixed summation tree
    const int chunk = blockIdx.x, c = blockIdx.y, nc = gridDim.y, D = S.D, tid = threadIdx.x;
    nrows = min(nrows, S.Ncap + S.ctl->nphantom);   // the grid may have been sized before the phantoms were cleaned
    const int r0 = chunk * CR, r1 = min(nrows, r0 + CR);
    const int DPc = cov_dpc(D), G = 256 / DPc, g = tid / DPc;
    __shared__ int rc[PC_COV_ROWS];
    __shared__ double red[256];
    int mine = 0;
    for (int r = r0 + tid; r < r1; r += 256) { int cc; cov_row(S, r, S.Ncap, nc, cc); rc[r - r0] = cc; mine += (cc == c); }
    const int cnt = __syncthreads_count(mine);
    for (int d = tid % DPc; d < D; d += DPc) {
        double s = 0.0;
        int r = r0 + g;
        for (; r + 7 * G < r1; r += 8 * G) {              // eight independent loads in flight, added in row order
            double t8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t8[u] = (rc[r + u * G - r0] == c) ? cov_ptr(S, r + u * G)[d] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) s += t8[u];
        }
        for (; r < r1; r += G)
            if (rc[r - r0] == c) s += cov_ptr(S, r)[d];
        if (G > 1) red[tid] = s; else psum[((size_t)chunk * nc + c) * D + d] = s;
    }
    if (G > 1) {
        __syncthreads();
        if (tid < D) {
            double s = 0.0;
            for (int gg = 0; gg < G; ++gg) s += red[gg * DPc + tid];
            psum[((size_t)chunk * nc + c) * D + tid] = s;
        }
    }
    if (tid == 0) pcnt[(size_t)chunk * nc + c] = cnt;
}

__global__ __launch_bounds__(256) void k_cov_partial(PcState S, int nrows, int nchunk, const double *psum, const int *pcnt,
                                                    double *mean /* [nc][D] */, int *count /* [nc] */, double *pcov, int CR,
                                                    int TS /* tile row stride */, int use_mfma, int nchunk_rows)
{
    // grid (nchunk, nc).  Every workgroup first reduces the chunk sums to the cluster mean (fixed order,
    // identical in every workgroup), then accumulates the centred outer products of its own rows.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int chunk = blockIdx.x, c = blockIdx.y, nc = gridDim.y, D = S.D, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    nrows = min(nrows, S.Ncap + S.ctl->nphantom);
    double *tile = (double *)smem;               // [rows][TS], TS = D+1 or (D rounded up to 16)+1, zero padded
    double *mu = tile + (size_t)CR * TS;         // [D]
    double *red = mu + D;                        // [256]
    int *rc = (int *)(red + 256);                // [CR] member rows, in row order
    __shared__ int wcnt[4];
    __shared__ int nred[256];
    const int DPc = cov_dpc(D), G = 256 / DPc, g = tid / DPc;
    // ---- mean
    {
        int nn = 0;
        for (int k = tid; k < nchunk; k += 256) nn += pcnt[(size_t)k * nc + c];
        nred[tid] = nn;
    }
    for (int d = tid % DPc; d < D; d += DPc) {
        double s = 0.0;
        PC_STRIDED_SUM(s, g, nchunk, G, k, psum[((size_t)k * nc + c) * D + d])
        if (G > 1) red[tid] = s; else mu[d] = s;
    }
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if (tid < off) nred[tid] += nred[tid + off]; __syncthreads(); }
    const int ntot = nred[0];
    if (G > 1 && tid < D) {
        double s = 0.0;
        for (int gg = 0; gg < G; ++gg) s += red[gg * DPc + tid];
        mu[tid] = s;
    }
    __syncthreads();
    for (int d = tid; d < D; d += 256) {
        const double m = mu[d] / (double)ntot;
        mu[d] = m;
        if (chunk == 0) mean[(size_t)c * D + d] = m;
    }
    if (chunk == 0 && tid == 0) count[c] = ntot;
    // ---- wide nDims: X^T X on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), upper triangle only, one 16x16 tile of
    // the result per wave at a time.  Operand maps (cdna_hip_programming.md): A[i=lane&15][k=lane>>4],
    // B[k=lane>>4][j=lane&15], D col = lane&15, row = (lane>>4) + 4*reg.  The workgroup is persistent: it takes the chunks
    // chunk, chunk + gridDim.x, ... and keeps its accumulators in registers across them, so that ONE partial matrix
    // per workgroup goes to memory (a 100-D update used to write and re-read one 80 KB partial per 128 rows: 1.3 GB).
    // Rows are consumed four at a time in row order, chunks in order: a fixed summation order.
    typedef double v4d __attribute__((ext_vector_type(4)));
    constexpr int MAXT = 9;                                       // tiles per wave: nDims <= 128 -> 36 tiles / 4 waves
    v4d acc[MAXT];
    const int W = TS - 1, nt = W / 16, ntile = nt * (nt + 1) / 2;
    // beyond 128 dimensions there are more result tiles than a wave's registers hold (136 at nDims = 256): the
    // workgroup walks its chunks once per group of 4 x MAXT tiles
    for (int tile0 = 0; tile0 == 0 || (use_mfma && tile0 < ntile); tile0 += 4 * MAXT) {
#pragma unroll
    for (int k = 0; k < MAXT; ++k) acc[k] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int ch = chunk; ch == chunk || (use_mfma && ch < nchunk_rows); ch += gridDim.x) {
    const int r0 = ch * CR, r1 = max(r0, min(nrows, r0 + CR));
    // ---- member rows of this chunk, in row order (CR <= 256: one row per thread)
    bool member = false;
    { const int r = r0 + tid; int cc = -1; if (tid < CR && r < r1) cov_row(S, r, S.Ncap, nc, cc); member = (tid < CR && r < r1 && cc == c); }
    const unsigned long long bm = __ballot(member);
    __syncthreads();                                              // the previous chunk's tile and rc are no longer read
    if (lane == 0) wcnt[wv] = __popcll(bm);
    __syncthreads();
    int base = 0;
    for (int x = 0; x < wv; ++x) base += wcnt[x];
    const int n = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (member) rc[base + __popcll(bm & ((1ull << lane) - 1ull))] = r0 + tid;
    __syncthreads();
    if (!use_mfma) {
        {
            int e = tid;
            for (; e + 7 * 256 < n * D; e += 8 * 256) {   // eight independent row reads in flight
                double t8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int ee = e + u * 256; t8[u] = cov_ptr(S, rc[ee / D])[ee % D]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int ee = e + u * 256, i = ee / D, d = ee % D; tile[(size_t)i * TS + d] = t8[u] - mu[d]; }
            }
            for (; e < n * D; e += 256) { const int i = e / D, d = e % D; tile[(size_t)i * TS + d] = cov_ptr(S, rc[i])[d] - mu[d]; }
        }
        __syncthreads();
        for (int p = tid; p < D * D; p += 256) {
            const int a = p / D, b = p % D;
            // rows i, i+1, i+2, i+3 on four accumulators (four independent rows to a pass)
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int i = 0;
            for (; i + 3 < n; i += 4) {
                s0 += tile[(size_t)i * TS + a] * tile[(size_t)i * TS + b];
                s1 += tile[(size_t)(i + 1) * TS + a] * tile[(size_t)(i + 1) * TS + b];
                s2 += tile[(size_t)(i + 2) * TS + a] * tile[(size_t)(i + 2) * TS + b];
                s3 += tile[(size_t)(i + 3) * TS + a] * tile[(size_t)(i + 3) * TS + b];
            }
            for (; i < n; ++i) s0 += tile[(size_t)i * TS + a] * tile[(size_t)i * TS + b];
            pcov[((size_t)chunk * nc + c) * D * D + p] = (s0 + s1) + (s2 + s3);
        }
        return;
    }
    const int nP = (n + 3) & ~3;                                  // rows of the zero padded tile
    for (int e = tid; e < nP * W; e += 256) {
        const int i = e / W, d = e % W;
        tile[(size_t)i * TS + d] = (i < n && d < D) ? cov_ptr(S, rc[i])[d] - mu[d] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
        const int t = tile0 + wv + 4 * k;
        if (t < ntile) {
            int ti = 0, rem = t;
            while (rem >= nt - ti) { rem -= nt - ti; ti++; }
            const int tj = ti + rem;
            const double *pa = tile + (size_t)(lane >> 4) * TS + ti * 16 + (lane & 15);
            const double *pb = tile + (size_t)(lane >> 4) * TS + tj * 16 + (lane & 15);
            v4d a4 = acc[k];
            for (int q0 = 0; q0 < nP; q0 += 4)
                a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[(size_t)q0 * TS], pb[(size_t)q0 * TS], a4, 0, 0, 0);
            acc[k] = a4;
        }
    }
    }   // chunks of this workgroup
    double *out = pcov + ((size_t)chunk * nc + c) * D * D;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
        const int t = tile0 + wv + 4 * k;
        if (t < ntile) {
            int ti = 0, rem = t;
            while (rem >= nt - ti) { rem -= nt - ti; ti++; }
            const int tj = ti + rem;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = ti * 16 + (lane >> 4) + 4 * r, col = tj * 16 + (lane & 15);
                if (row < D && col < D) { out[(size_t)row * D + col] = acc[k][r]; if (ti != tj) out[(size_t)col * D + row] = acc[k][r]; }
            }
        }
    }
    }   // groups of tiles
}

// Fold the per-chunk partial sums of a cluster into the first R chunk slots (slot r = chunks r, r+R, ... added in
// that order; slot r is only ever read by workgroup r, so the fold is in place).  A 100-D run has ~800 chunks
// of 80 KB each: one workgroup reading all of them for the final sum took 3 ms per update.
__global__ __launch_bounds__(256) void k_fold_partials(double *buf, int *cnt, int nchunk, int nc, int per)
{
    const int r = blockIdx.x, R = gridDim.x, c = blockIdx.y, tid = threadIdx.x;
    for (int p = tid; p < per; p += 256) {
        double s = 0.0;
        PC_STRIDED_SUM(s, r, nchunk, R, k, buf[((size_t)k * nc + c) * per + p])
        buf[((size_t)r * nc + c) * per + p] = s;
    }
    if (cnt && tid == 0) {
        int n = 0;
        for (int k = r; k < nchunk; k += R) n += cnt[(size_t)k * nc + c];
        cnt[(size_t)r * nc + c] = n;
    }
}

#define PC_CHOL_NT 1024
__global__ __launch_bounds__(PC_CHOL_NT) void k_cov_final_chol(PcState S, int nchunk, const double *pcov, const int *count, int a_global, int only_if_suspect)
{
    if (only_if_suspect && !S.ctl->chol_suspect) return;          // (uniform) the blocked factorisation in front of this launch stands
    // one workgroup per cluster: fixed-order sum of the partials, then calc_cholesky (utils.F90:621-649)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int c = blockIdx.x, nc = gridDim.x, D = S.D, DD = D * D, tid = threadIdx.x;
    // red [PC_CHOL_NT]: scratch of the reduction; it borrows L (zeroed afterwards) when the two matrices
    // alone fill the LDS (nDims = 100: 2 x 80 KB)
    // a_global (nDims > 101: two matrices exceed the LDS): the covariance is read back from S.cov, only L lives in LDS
    // a_global == 2 (nDims > 143: not even L fits): the factor is built in place in S.chol, the LDS holds the scratch only
    double *A = a_global ? S.cov + (size_t)c * DD : (double *)smem;
    double *L = a_global == 2 ? S.chol + (size_t)c * DD : (a_global ? (double *)smem : A + DD);
    double *red = a_global == 2 ? (double *)smem : ((DD >= PC_CHOL_NT) ? L : L + DD);
    __shared__ int bad;
    const double n = (double)count[c];
    // G groups of DDp threads; group g adds chunks g, g+G, ... in order, then the groups are added in order
    int DDp = (DD + 63) & ~63;
    if (DDp > PC_CHOL_NT) DDp = PC_CHOL_NT;
    const int G = PC_CHOL_NT / DDp, g = tid / DDp;
    for (int p0 = 0; p0 < DD; p0 += DDp) {
        const int p = p0 + tid % DDp;
        double s = 0.0;
        if (p < DD && g < G) PC_STRIDED_SUM(s, g, nchunk, G, k, pcov[((size_t)k * nc + c) * DD + p])
        red[tid] = s;
        __syncthreads();
        if (tid < DDp && p < DD) {
            double t = 0.0;
            for (int gg = 0; gg < G; ++gg) t += red[gg * DDp + tid];
            const double av = t / n;
            if (!a_global) A[p] = av;
            S.cov[(size_t)c * DD + p] = av;
        }
        __syncthreads();
    }
    for (int p = tid; p < DD; p += PC_CHOL_NT) L[p] = 0.0;
    if (tid == 0) bad = 0;
    __syncthreads();
    // calc_cholesky by ONE wavefront, lane = row: column i needs, for every row j >= i, the dot product
    // sum_{k<i} L(i,k) L(j,k) in ascending k (the reference's order); row i's own value gives the
    // diagonal.  No workgroup barrier inside the column loop, only wave-level LDS ordering.
    if (a_global == 2) {
        // The factor is built TRANSPOSED in HBM (L(j,k) at [k][j]): lane = row, so a wave reads one contiguous stretch per
        // k instead of 64 cache lines, the four rows a lane owns are four independent sums in the same ascending-k order,
        // and a column is stored as one contiguous row.  Transposed in place at the end.
        if (tid < 64) {
            for (int i = 0; i < D; ++i) {
                double tj[4] = {0.0, 0.0, 0.0, 0.0};
                int jc[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) jc[m] = min(m * 64 + tid, D - 1);     // rows past D: a harmless duplicate
                int k = 0;
                for (; k + 8 <= i; k += 8) {                 // forty loads in flight, then the sums in ascending k
                    double lik[8], l4[8][4];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const double *Lk = L + (size_t)(k + u) * D;
                        lik[u] = Lk[i];
#pragma unroll
                        for (int m = 0; m < 4; ++m) l4[u][m] = Lk[jc[m]];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int m = 0; m < 4; ++m) tj[m] += lik[u] * l4[u][m];
                }
                for (; k < i; ++k) {
                    const double *Lk = L + (size_t)k * D;
                    const double lik = Lk[i];
#pragma unroll
                    for (int m = 0; m < 4; ++m) tj[m] += lik * Lk[jc[m]];
                }
                double ti = 0.0;
#pragma unroll
                for (int m = 0; m < 4; ++m) { const double v = __shfl(tj[m], i & 63); if ((i >> 6) == m) ti = v; }
                const double dii = A[i * D + i] - ti;
                if (dii <= 0.0) { if (tid == 0) bad = 1; break; }
                const double lii = sqrt(dii);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int j = m * 64 + tid;
                    if (j > i && j < D) L[(size_t)i * D + j] = (A[i * D + j] - tj[m]) / lii;
                }
                if (tid == 0) L[(size_t)i * D + i] = lii;
                __threadfence_block();
            }
        }
        __syncthreads();
        if (!bad)
            for (int p = tid; p < DD; p += PC_CHOL_NT) {
                const int a = p / D, b = p % D;
                if (a < b) { const double x = L[p], y = L[(size_t)b * D + a]; L[p] = y; L[(size_t)b * D + a] = x; }
            }
    }
    else if (tid < 64) {
        for (int i = 0; i < D; ++i) {
            double tj[4] = {0.0, 0.0, 0.0, 0.0};           // D <= 256: at most 4 rows per lane
            #pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int j = m * 64 + tid;
                if (j >= i && j < D) {
                    double t = 0.0;
                    for (int k = 0; k < i; ++k) t += L[i * D + k] * L[j * D + k];
                    tj[m] = t;
                }
            }
            double ti = 0.0;                                // row i's own dot product
            #pragma unroll
            for (int m = 0; m < 4; ++m) { const double v = __shfl(tj[m], i & 63); if ((i >> 6) == m) ti = v; }
            const double dii = A[i * D + i] - ti;
            if (dii <= 0.0) { if (tid == 0) bad = 1; break; }
            const double lii = sqrt(dii);
            #pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int j = m * 64 + tid;
                if (j > i && j < D) L[j * D + i] = (A[i * D + j] - tj[m]) / lii;
            }
            if (tid == 0) L[i * D + i] = lii;
            __threadfence_block();
        }
    }
    __syncthreads();
    if (bad && tid == 0 && (S.ablate & PC_ABL_TRACE_CHOL)) printf("engine chol fallback: cluster %d of %d, n = %d\n", c, nc, (int)n);   // developer trace
    if (bad) {   // no Cholesky factor: scaled identity (utils.F90:633-638)
        double tr = 0.0;
        for (int k = 0; k < D; ++k) tr += A[k * D + k];
        for (int p = tid; p < DD; p += PC_CHOL_NT) L[p] = (p / D == p % D) ? sqrt(tr) : 0.0;
    }
    __syncthreads();
    if (a_global != 2) for (int p = tid; p < DD; p += PC_CHOL_NT) S.chol[(size_t)c * DD + p] = L[p];
}

// calc_cholesky (utils.F90:621-649) for 32 <= nDims <= 128, one cluster, as a blocked right-looking factorisation: panels of
// sixteen columns -- the 16 x 16 diagonal block by one wave with a row per lane in registers, the rows below it by forward
// substitution (a thread per row), the trailing matrix A22 -= L21 L21^T in 16 x 16 tiles on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64, four contraction steps per tile and panel) -- with the matrix in LDS throughout.  The reference
// sums its dot products in ascending k, one column at a time; this sums the same products panel by panel: the factor agrees to
// round-off.  Where that is not good enough -- a pivot that is not clearly positive, i.e. a covariance that is singular to
// working precision, where round-off decides whether the reference falls back to the scaled identity (utils.F90:633-638) --
// the kernel says so (PcCtl::chol_suspect) and the reference-order kernel launched behind it redoes the factorisation;
// otherwise that launch returns at once.  One-wave kernel: 0.35 ms per update at nDims = 100, this: 0.03.
template <int NT>
__global__ __launch_bounds__(256) void k_chol_blocked(PcState S, const double *ncov, const int *count)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef double v4d __attribute__((ext_vector_type(4)));
    constexpr int NR = 16 * NT, NS = NR + 1;
    double *A = (double *)smem;                                         // [NR][NS]
    __shared__ int suspect;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4, D = S.D;
    const double n = (double)count[0];
    for (int e = tid; e < NR * NR; e += 256) {
        const int i = e / NR, j = e - i * NR;
        double v = (i == j) ? 1.0 : 0.0;                                // rows and columns beyond nDims: identity
        if (i < D && j < D) { v = ncov[(size_t)i * D + j] / n; S.cov[(size_t)i * D + j] = v; }
        A[i * NS + j] = v;
    }
    if (tid == 0) suspect = 0;
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < NT; ++p) {
        const int c0 = 16 * p;
        // ---- diagonal block: lane = row, right-looking in registers
        if (wv == 0) {
            double a[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = A[(c0 + li) * NS + c0 + k];
            bool bad = false;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const double aii = readlane_f64(a[i], i);
                if (!(aii > 0.0)) bad = true;
                const double lii = sqrt(fabs(aii) + (aii > 0.0 ? 0.0 : 1.0));
                const double lji = (li == i) ? lii : a[i] / lii;
                if (li >= i) a[i] = lji;
#pragma unroll
                for (int k = i + 1; k < 16; ++k) { const double lki = readlane_f64(lji, k); if (li > i) a[k] -= lji * lki; }
            }
            if (lk == 0) {
#pragma unroll
                for (int k = 0; k < 16; ++k) A[(c0 + li) * NS + c0 + k] = (k <= li) ? a[k] : 0.0;
            }
            if (bad && lane == 0) suspect = 1;
        }
        __syncthreads();
        // ---- rows below: x L11^T = A21, a thread per row
        {
            const int i = c0 + 16 + tid;
            if (i < NR) {
                double x[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    double s = A[i * NS + c0 + j];
#pragma unroll
                    for (int k = 0; k < j; ++k) s -= x[k] * A[(c0 + j) * NS + c0 + k];
                    x[j] = s / A[(c0 + j) * NS + c0 + j];
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) A[i * NS + c0 + j] = x[j];
            }
        }
        __syncthreads();
        // ---- trailing matrix, lower triangle of tiles, dealt out to the four waves
        int q = 0;
        for (int ti = p + 1; ti < NT; ++ti)
            for (int tj = p + 1; tj <= ti; ++tj, ++q) {
                if ((q & 3) != wv) continue;
                v4d acc;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = A[(16 * ti + lk + 4 * r) * NS + 16 * tj + li];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[(16 * ti + li) * NS + c0 + 4 * ks + lk], A[(16 * tj + li) * NS + c0 + 4 * ks + lk], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) A[(16 * ti + lk + 4 * r) * NS + 16 * tj + li] = acc[r];
            }
        __syncthreads();
    }
    // a pivot that is tiny against its own diagonal element is round-off's to decide as well
    for (int i = tid; i < D; i += 256) { const double l = A[i * NS + i]; if (!(l * l > 1e-9 * S.cov[(size_t)i * D + i])) suspect = 1; }
    __syncthreads();
    if (tid == 0) S.ctl->chol_suspect = suspect;
    if (suspect) return;
    for (int e = tid; e < D * D; e += 256) { const int i = e / D, j = e - i * D; S.chol[e] = (j <= i) ? A[i * NS + j] : 0.0; }
}

// ------------------------------------------------------------------------------------------
// posterior moments of theta from the dead points: weights exp(logw + logL - max), fixed-order sums about a pivot (the row of
// the largest weight, lowest index on ties), so that the variance of a narrow posterior far from zero keeps its digits
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void post_argmax(double &m, int &im, double om, int oi)
{
    if (om > m || (om == m && oi < im)) { m = om; im = oi; }
}
// pmax[b] = largest posterior log-weight of block b's rows, pmax[grid + b] = its row (as a double; -1: none)
__global__ __launch_bounds__(256) void k_post_max(PcState S, int nd, double *pmax)
{
    __shared__ double red[256];
    __shared__ int redi[256];
    if (nd < 0) nd = S.ctl->ndead;                      // (enqueued behind the kill-off, before the host knows the count)
    double m = -PC_HUGE;
    int im = 0x7fffffff;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nd; i += gridDim.x * 256) {
        const double lw = S.dead_logw[i];
        if (lw > S.logzero) post_argmax(m, im, lw + S.dead[(size_t)i * S.nT + S.l0], i);
    }
    red[threadIdx.x] = m; redi[threadIdx.x] = im;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) { double a = red[threadIdx.x]; int ia = redi[threadIdx.x]; post_argmax(a, ia, red[threadIdx.x + off], redi[threadIdx.x + off]); red[threadIdx.x] = a; redi[threadIdx.x] = ia; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { pmax[blockIdx.x] = red[0]; pmax[gridDim.x + blockIdx.x] = redi[0] == 0x7fffffff ? -1.0 : (double)redi[0]; }
}

__global__ __launch_bounds__(256) void k_post_moments(PcState S, int nd, const double *pmax, double *part /* [grid][3D+1] */)
{
    // thread = (row group g, coordinate d); group g takes rows blockIdx*G+g, +gridDim*G, ... in order.
    // part[b] = sum w (x - p) [D], sum w (x - p)^2 [D], sum w, p [D]
    __shared__ double red[256];
    __shared__ double red2[256];
    __shared__ int redi[256];
    const int tid = threadIdx.x, D = S.D + S.nDer;          // theta then phi, contiguous from p0
    const int DPc = cov_dpc(D), G = 256 / DPc, g = tid / DPc, pw = 3 * D + 1;
    if (nd < 0) nd = S.ctl->ndead;
    double m = -PC_HUGE;
    int im = 0x7fffffff;
    for (int b = tid; b < (int)gridDim.x; b += 256) { const double ib = pmax[gridDim.x + b]; if (ib >= 0.0) post_argmax(m, im, pmax[b], (int)ib); }
    red[tid] = m; redi[tid] = im;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { double a = red[tid]; int ia = redi[tid]; post_argmax(a, ia, red[tid + off], redi[tid + off]); red[tid] = a; redi[tid] = ia; }
        __syncthreads();
    }
    m = red[0];
    const double *prow = (redi[0] < nd) ? S.dead + (size_t)redi[0] * S.nT + S.p0 : nullptr;
    __syncthreads();
    for (int d0 = 0; d0 < D; d0 += DPc) {
        const int d = d0 + tid % DPc;
        const double p = (d < D && prow) ? prow[d] : 0.0;
        double s1 = 0.0, s2 = 0.0, sw = 0.0;
        for (int i = blockIdx.x * G + g; i < nd; i += gridDim.x * G) {
            const double lw = S.dead_logw[i];
            if (!(lw > S.logzero)) continue;
            const double *row = S.dead + (size_t)i * S.nT;
            const double wgt = exp(lw + row[S.l0] - m);
            sw += wgt;
            if (d < D) { const double th = row[S.p0 + d] - p; s1 += wgt * th; s2 += wgt * th * th; }
        }
        red[tid] = s1; red2[tid] = s2;
        __syncthreads();
        if (tid < DPc && d < D) {
            double a = 0.0, b2 = 0.0;
            for (int gg = 0; gg < G; ++gg) { a += red[gg * DPc + tid]; b2 += red2[gg * DPc + tid]; }
            part[(size_t)blockIdx.x * pw + d] = a; part[(size_t)blockIdx.x * pw + D + d] = b2; part[(size_t)blockIdx.x * pw + 2 * D + 1 + d] = p;
        }
        __syncthreads();
        if (d0 == 0) {
            red[tid] = (tid % DPc == 0) ? sw : 0.0;
            __syncthreads();
            if (tid == 0) { double a = 0.0; for (int gg = 0; gg < G; ++gg) a += red[gg * DPc]; part[(size_t)blockIdx.x * pw + 2 * D] = a; }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
// phantom clean: returns nothing; *d_total (device int) receives the surviving count
extern "C" void pc_launch_clean(const PcState *S, int nph, unsigned char *keep, int *blk, int *d_total, double *ph2,
                                double *phL2, unsigned *phC2, unsigned long long *phU2, int *dst_index, hipStream_t st)
{
    const int nblk = (nph + 255) / 256;
    if (nblk > 0) {
        hipLaunchKernelGGL(k_clean_flag, dim3(nblk), dim3(256), 0, st, *S, nph, keep, blk);
        hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, st, blk, nblk, d_total, &S->ctl->nphantom);
        hipLaunchKernelGGL(k_clean_scatter, dim3(nblk), dim3(256), 0, st, *S, nph, keep, blk, ph2, phL2, phC2, phU2, dst_index);
    } else {
        hipMemsetAsync(d_total, 0, sizeof(int), st);
        hipMemsetAsync(&S->ctl->nphantom, 0, sizeof(int), st);
    }
}

// the phantom clean for R runs at once (pool compaction of runs in step): every run its own row count (PcManyRec::ia[PC_REC_I_ROWS], blocks PC_REC_I_BLOCKS)
extern "C" int pc_launch_clean_many(const PcManyRec *dR, int R, int nblk_max, hipStream_t st)
{
    if (nblk_max < 1) return 1;
    hipLaunchKernelGGL(k_clean_flag_many, dim3(nblk_max, R), dim3(256), 0, st, dR);
    hipLaunchKernelGGL(k_scan_blocks_many, dim3(1, R), dim3(256), 0, st, dR);
    hipLaunchKernelGGL(k_clean_scatter_many, dim3(nblk_max, R), dim3(256), 0, st, dR);
    return 0;
}

extern "C" void pc_launch_reset_thresholds(const PcState *S, hipStream_t st)
{
    hipLaunchKernelGGL(k_reset_thresholds, dim3(1), dim3(S->maxc <= 1024 ? ((S->maxc + 63) / 64) * 64 : 1024), 0, st, *S);
}

extern "C" int pc_launch_reset_thresholds_many(const PcState *S, const PcManyRec *dR, int R, hipStream_t st)
{
    (void)S;
    hipLaunchKernelGGL(k_reset_thresholds_many, dim3(1, R), dim3(256), 0, st, dR);
    return 0;
}

static int cov_use_mfma(const PcState *S) { return S->D >= 32; }
static int cov_tile_stride(const PcState *S) { return cov_use_mfma(S) ? ((S->D + 15) & ~15) + 1 : S->D + 1; }
static int cov_rows(const PcState *S)
{   // rows per chunk: the centred tile [rows][stride] must fit in LDS
    int r = PC_COV_ROWS;
    while (r > 8 && sizeof(double) * (size_t)r * cov_tile_stride(S) + sizeof(int) * r > 120 * 1024) r >>= 1;
    return r;
}
extern "C" int pc_cov_nchunk(const PcState *S, int nph) { const int r = cov_rows(S); return (S->Ncap + nph + r - 1) / r; }
// where k_cov_final_chol keeps its matrices (its a_global: 0 both in LDS, 1 the covariance read back from S.cov, 2 the factor in place in S.chol
// as well) and the dynamic LDS that takes: the first of the three that fits in 160 KB
struct CholLayout { int a_global; size_t lds; };
static CholLayout chol_layout(int D)
{
    const size_t DD = (size_t)D * D, red = DD >= PC_CHOL_NT ? 0 : PC_CHOL_NT;      // (red: the reduction's scratch borrows L where L is that large)
    if (sizeof(double) * (2 * DD + red) <= 160 * 1024) return {0, sizeof(double) * (2 * DD + red)};
    if (sizeof(double) * (DD + red) <= 160 * 1024) return {1, sizeof(double) * (DD + red)};
    return {2, sizeof(double) * PC_CHOL_NT};
}

extern "C" int pc_launch_covmats(const PcState *S, int nph, int nc, double *psum, int *pcnt, double *mean, int *count,
                                 double *pcov, hipStream_t st)
{
    const int CR = cov_rows(S);
    const int nrows = S->Ncap + nph, nchunk = (nrows + CR - 1) / CR, D = S->D;
    hipLaunchKernelGGL(k_cov_mean_partial, dim3(nchunk, nc), dim3(256), 0, st, *S, nrows, nph, psum, pcnt, CR);
    const int NFOLD = 64;
    int nred = nchunk;                                           // partial sums the later stages read
    if (nchunk > 2 * NFOLD) {
        hipLaunchKernelGGL(k_fold_partials, dim3(NFOLD, nc), dim3(256), 0, st, psum, pcnt, nchunk, nc, D);
        nred = NFOLD;
    }
    const int TS = cov_tile_stride(S);
    const size_t sh = sizeof(double) * ((size_t)CR * TS + D + 256) + sizeof(int) * CR;
    if (sh > 160 * 1024) return 1;
    pc_need_dyn_lds((const void *)k_cov_partial, sh);
    int ncov = nred;                                             // partial matrices the Cholesky kernel adds up
    if (cov_use_mfma(S)) {
        // persistent workgroups (one per CU at nDims = 100), each walks its share of the chunks and writes one partial matrix
        const int G = nchunk < 256 ? nchunk : 256;
        hipLaunchKernelGGL(k_cov_partial, dim3(G, nc), dim3(256), sh, st, *S, nrows, nred, psum, pcnt, mean, count, pcov, CR, TS, 1, nchunk);
        ncov = G;
    } else {
        hipLaunchKernelGGL(k_cov_partial, dim3(nchunk, nc), dim3(256), sh, st, *S, nrows, nred, psum, pcnt, mean, count, pcov, CR, TS, 0, nchunk);
        if (nchunk > 2 * NFOLD) hipLaunchKernelGGL(k_fold_partials, dim3(NFOLD, nc), dim3(256), 0, st, pcov, (int *)nullptr, nchunk, nc, D * D);
    }
    const CholLayout cl = chol_layout(D);
    pc_need_dyn_lds((const void *)k_cov_final_chol, cl.lds);
    hipLaunchKernelGGL(k_cov_final_chol, dim3(nc), dim3(PC_CHOL_NT), cl.lds, st, *S, ncov, pcov, count, cl.a_global, 0);
    return 0;
}

// pieces of the general update path used by the fused update of pc_update.hip
extern "C" void pc_launch_scan_blocks(int *blk, int nblk, int *total, int *total2, hipStream_t st)
{
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, st, blk, nblk, total, total2);
}
extern "C" void pc_launch_chol_only(const PcState *S, const double *ncov, const int *count, hipStream_t st)
{   // one cluster, one "partial" = n times the covariance
    const int D = S->D;
    const CholLayout cl = chol_layout(D);
    pc_need_dyn_lds((const void *)k_cov_final_chol, cl.lds);
    static const bool blocked_off = std::getenv("PC_CHOL_BLOCKED_OFF") != nullptr;
    int guard = 0;
    if (!blocked_off && D >= 32 && D <= 128) {
        const int nt = (D + 15) / 16;
        const size_t shb = sizeof(double) * (size_t)(16 * nt) * (16 * nt + 1);
#define PC_CHOLB(NT) { pc_need_dyn_lds((const void *)k_chol_blocked<NT>, shb); \
            hipLaunchKernelGGL((k_chol_blocked<NT>), dim3(1), dim3(256), shb, st, *S, ncov, count); }
        switch (nt) { case 2: PC_CHOLB(2) break; case 3: PC_CHOLB(3) break; case 4: PC_CHOLB(4) break; case 5: PC_CHOLB(5) break;
                      case 6: PC_CHOLB(6) break; case 7: PC_CHOLB(7) break; default: PC_CHOLB(8) break; }
#undef PC_CHOLB
        guard = 1;
    }
    hipLaunchKernelGGL(k_cov_final_chol, dim3(1), dim3(PC_CHOL_NT), cl.lds, st, *S, 1, ncov, count, cl.a_global, guard);
}

#define PC_POST_BLOCKS 512
extern "C" int pc_post_blocks(void) { return PC_POST_BLOCKS; }
extern "C" void pc_launch_post_moments(const PcState *S, int nd, double *pmax, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(k_post_max, dim3(PC_POST_BLOCKS), dim3(256), 0, st, *S, nd, pmax);
    hipLaunchKernelGGL(k_post_moments, dim3(PC_POST_BLOCKS), dim3(256), 0, st, *S, nd, pmax, part);
}
