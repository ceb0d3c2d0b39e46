// pc_quad_mm.hip -- the batched quadratic form (pchip_source_create_quad_batch): chi2 = r^T P r of MANY points at once on the fp64 matrix cores.
//
// A round of the device batch path (Engine::slice_device, pc_engine.hip) parks hundreds to thousands of proposals; their residuals together are
// a matrix R [n][nres], and  chi2_k = sum_j R[k][j] * (sum_i R[k][i] * P[i][j])  is the diagonal of (R P) R^T: a matrix-matrix product with a
// fused epilogue.  Three launches a call (pc_launch_quad_batch): k_quad_residuals and k_quad_finish call the user's functions and live in the
// handle's run-time module (pc_sample.hip under PCHIP_USER_QUAD_BATCH); k_quad_chi2_mm, between them, is this file's static kernel.
//
// THE CONTRACT (tests/test_source_quad_batch.py rests on it):
//   * A row's bits depend on that row's residuals, on P and on nres ONLY -- not on n, not on the row's place in the block, not on what the
//     other rows hold.  The split of columns over wavefronts and workgroups is a function of nres alone (pc_quad_mm_ncb); the contraction
//     index advances in the same steps of four from 0 for every row; ragged edges are zero OPERANDS (residual padding written by
//     k_quad_residuals, matrix elements beyond nres loaded as 0.0), never another code path for some rows; an accumulator element of the
//     matrix instruction depends on its own row of A alone.
//   * P is used exactly as given: row-major at data + ndata (8-byte aligned, read by 8-byte loads), not symmetrised, not transposed.
//   * nres and n are free: any 1 <= nres <= PCHIP_SOURCE_MAX_RES_BATCH, any n >= 1.
//
// The order of one row k's arithmetic:
//   1. q_j = the accumulator of v_mfma_f64_16x16x4_f64 over i = 0, 4, 8, ... (the instruction's own order inside a step of four), up to
//      nres rounded up to 16 -- the tail multiplies zeros;
//   2. t_j = q_j * R[k][j], one IEEE multiply, kept from fusing with the adds behind it;
//   3. the sixteen t_j of a column tile by row_sum's butterfly over lane & 15 (pc_dev.h: xor 1, xor 2, half mirror, mirror);
//   4. a wavefront adds its two column tiles in ascending order and writes part[k][32-column strip];
//   5. k_quad_finish adds a row's pc_quad_mm_ncb(nres) partials in ascending order to 0.0.  No atomics on doubles anywhere.
//
// Shape, reasoned (not measured): Q = R P costs 2 n nres^2 flop -- 8.4 Gflop at nres = 2048, n = 1000, 0.1 ms at the 78.6 Tflop/s fp64 matrix
// peak -- and P is read once per block of rows: with 64 rows a workgroup 16 x 32 MB = 0.5 GB, about the same time from HBM, most of it
// from L2 in fact (all column blocks of one row block run side by side).  So a workgroup takes 64 rows x 128 columns: four wavefronts, each a
// strip of 32 columns (two column tiles) under all four row tiles, eight 16 x 16 accumulators, 64 registers.  A matrix element is needed
// by ONE wavefront of the workgroup (the strips are disjoint), for four row tiles out of one register: staging P through LDS would buy
// no reuse, its loads go straight to registers, sixteen consecutive doubles a row of lanes, a whole chunk of sixteen rows in flight ahead of
// the barrier.  R is what the four wavefronts share: its 64 x 16 chunk goes through LDS, double-buffered, one barrier a chunk, rows 20 doubles
// apart (the sixty-four 8-byte reads of an A operand then fall two to a bank pair, the minimum).  The grid splits the columns as well
// (nres / 128 column blocks): at n = 256 there are only four row blocks, and the partials make the split free.
#include "pc_state.h"
#include "pc_launch.h"

typedef double qmm_v4d __attribute__((ext_vector_type(4)));
typedef double qmm_v2d __attribute__((ext_vector_type(2)));

constexpr int QMM_RB = PC_QUAD_MM_ROWS;      // rows a workgroup: four row tiles
constexpr int QMM_CB = 128;                  // columns a workgroup: four wavefronts x two column tiles
constexpr int QMM_KC = 16;                   // the contraction's chunk: ldr is a multiple of it, so a chunk of R is always whole
constexpr int QMM_LD = QMM_KC + 4;           // a row of the LDS chunk, in doubles

__global__ __launch_bounds__(256) void k_quad_chi2_mm(const double *__restrict__ R, const double *__restrict__ P, int nres, int ldr, int ncb,
                                                      double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) double Rs[2][QMM_RB * QMM_LD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, li = lane & 15, lk = lane >> 4;
    const int row0 = blockIdx.y * QMM_RB, col0 = blockIdx.x * QMM_CB + wv * 32;
    qmm_v4d acc[4][2];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = qmm_v4d{0.0, 0.0, 0.0, 0.0};
    // staging: thread t brings four consecutive doubles of row t / 4 of the chunk (ldr a multiple of 16, the block on 256 bytes: 16-byte loads)
    const int srow = t >> 2, sseg = (t & 3) * 4;
    const double *rsrc = R + (size_t)(row0 + srow) * ldr + sseg;
    const int nchunk = ldr / QMM_KC;
    for (int c = 0; c < nchunk; ++c) {
        const int i0 = c * QMM_KC;
        const qmm_v2d ra = *(const qmm_v2d *)(rsrc + i0), rb = *(const qmm_v2d *)(rsrc + i0 + 2);
        // the B operands of the chunk: lane (li, lk) holds P[i0 + 4 s + lk][col + li]; beyond nres in either index a zero
        double b[4][2];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int i = i0 + 4 * s + lk, j = col0 + 16 * ct + li;
                b[s][ct] = (i < nres && j < nres) ? P[(size_t)i * nres + j] : 0.0;
            }
        double *dst = Rs[c & 1] + srow * QMM_LD + sseg;
        *(qmm_v2d *)dst = ra; *(qmm_v2d *)(dst + 2) = rb;
        __syncthreads();      // (one a chunk: the buffer written now was last read before the barrier of the chunk in front)
        const double *as = Rs[c & 1] + li * QMM_LD + lk;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            double a[4];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) a[rt] = as[16 * rt * QMM_LD + 4 * s];      // A: lane (li, lk) holds R[row0 + 16 rt + li][i0 + 4 s + lk]
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], b[s][ct], acc[rt][ct], 0, 0, 0);
        }
    }
    // the epilogue: register r of lane (li, lk) is Q[row0 + 16 rt + lk + 4 r][col + li]
    const int strip = blockIdx.x * 4 + wv;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 16 * rt + lk + 4 * r;
            const double *rr = R + (size_t)row * ldr;
            const int j0 = col0 + li, j1 = col0 + 16 + li;
            double t0 = acc[rt][0][r] * (j0 < ldr ? rr[j0] : 0.0), t1 = acc[rt][1][r] * (j1 < ldr ? rr[j1] : 0.0);
            asm volatile("" : "+v"(t0)); asm volatile("" : "+v"(t1));
            row_sum2(t0, t1);
            const double s = t0 + t1;
            if (li == 0) part[(size_t)row * ncb + strip] = s;
        }
}

extern "C" int pc_launch_quad_chi2_mm(int n, int nres, const double *R, const double *P, double *part, hipStream_t st)
{
    if (n < 1 || nres < 1 || nres > PCHIP_SOURCE_MAX_RES_BATCH || !R || !P || !part) return 1;
    const long rows = pc_quad_mm_rows(n);
    if (rows / QMM_RB > 65535) return 1;      // (grid.y; the callers send at most PC_QUAD_BATCH_SLAB rows a call)
    const dim3 grid((unsigned)((nres + QMM_CB - 1) / QMM_CB), (unsigned)(rows / QMM_RB));
    hipLaunchKernelGGL(k_quad_chi2_mm, grid, dim3(256), 0, st, R, P, nres, pc_quad_mm_ldr(nres), pc_quad_mm_ncb(nres), part);
    return 0;
}

// the three launches for n rows: S is a source state of the handle (PC_LIKE_SOURCE, src_id, src_data / src_ndata, D, nDer)
extern "C" int pc_launch_quad_batch(const PcState *S, int nres, int n, const double *thetas, double *logL, double *phi, double *R, double *part, hipStream_t st)
{
    if (S->like.kind != PC_LIKE_SOURCE || n < 1 || nres < 1 || !S->src_data) return 1;
    const int ldr = pc_quad_mm_ldr(nres), ncb = pc_quad_mm_ncb(nres);
    const long rows = pc_quad_mm_rows(n);
    const long long cells = (long long)rows * ldr;
    if (cells > 0x7fffffffLL * 256) return 1;
    PcState s = *S;
    void *a1[] = { (void *)&s, (void *)&n, (void *)&thetas, (void *)&R };
    if (pc_rtc_launch(S, "k_quad_residuals", dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a1)) return 1;
    if (pc_launch_quad_chi2_mm(n, nres, R, S->src_data + S->src_ndata, part, st)) return 1;
    const double *cpart = part;
    void *a3[] = { (void *)&s, (void *)&n, (void *)&thetas, (void *)&cpart, (void *)&ncb, (void *)&logL, (void *)&phi };
    return pc_rtc_launch(S, "k_quad_finish", dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a3);
}
