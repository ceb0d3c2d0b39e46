// pc_park.hip -- the device batch callback's side of a round (polychord_hip_set_device_batch_callback): what k_slice_tick<true> parked is
// packed into one dense block in device memory, in ascending chain order, and handed to the caller's function as device pointers.
//
//   k_park_index   one workgroup: rank[c] = how many chains below c wait for an answer (-1 for a chain that does not), and their number
//                  to a device word and to ONE pinned host word -- all the host reads of a round;
//   k_park_rows    one wavefront a chain, lane = coordinate: the chain's parked cube to row rank[c] of the block;
//   k_park_index_many / k_park_rows_many   the same for a group of runs in step: the runs' rows one behind the other in ONE block, in the
//                  order of the runs, the ranks global, every run's count and the total to pinned words;
//   k_live_cubes   the prior samples of the live points, the Philox coordinates of generate_live_callback (PC_DOM_LIVEGEN, 0, attempt, d);
//   k_live_gather  the valid ones of them as rows [cube | theta | phi | logzero | logL] for pc_launch_install_live.
//
// The order is part of the contract: a caller's batched product may round by row position, and a run is reproducible.
#include "pc_state.h"
#include "pc_launch.h"

#define PC_PARK_THREADS 1024

// need: the chains' flags, flag of chain c at need[c * stride] (PcChain::need inside the chain records: pc_chain_need_layout; a plain
// array: stride 1).  Chunks of PC_PARK_THREADS chains: within a wavefront the rank is the population count of the ballot below the lane,
// across the wavefronts of a chunk the sum of their counts through LDS, across chunks a carry every thread keeps for itself.
__device__ __forceinline__ int park_ranks(int nchains, const int *need, int stride, int *rank)
{
    __shared__ int wave_n[PC_PARK_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int c0 = 0; c0 < nchains; c0 += PC_PARK_THREADS) {
        const int c = c0 + tid;
        const bool f = c < nchains && need[(size_t)c * stride] != 0;
        const unsigned long long m = pc_lanes(f);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PC_PARK_THREADS / 64; ++w) { const int n = wave_n[w]; before += w < wave ? n : 0; total += n; }
        if (c < nchains) rank[c] = f ? carry + before + below : -1;
        carry += total;
        __syncthreads();                                // wave_n is written again by the next chunk
    }
    return carry;
}

__global__ __launch_bounds__(PC_PARK_THREADS) void k_park_index(int nchains, const int *need, int stride, int *rank, int *count, int *count_host)
{
    const int carry = park_ranks(nchains, need, stride, rank);
    if (threadIdx.x == 0) { *count = carry; if (count_host) *count_host = carry; }
}

// The pack of a group of runs in step (pc_step.h): one workgroup a run, the scheme above for the run's LOCAL ranks, the run's number of parked
// chains to count[run] and to the pinned word count_host[run] (what the run reads to know whether it is done).
__global__ __launch_bounds__(PC_PARK_THREADS) void k_park_index_many(const PcParkRun *__restrict__ runs, int *count, int *count_host)
{
    const int run = blockIdx.x;
    const int carry = park_ranks(runs[run].nchains, pc_as_global(runs[run].need, runs), runs[run].stride, pc_as_global(runs[run].rank, runs));
    if (threadIdx.x == 0) { count[run] = carry; count_host[run] = carry; }
}

__global__ __launch_bounds__(64) void k_park_rows(int nchains, int D, const int *rank, const double *prop /* [nchains][D] */, double *cube /* [n][D] */)
{
    const int chain = blockIdx.x, lane = threadIdx.x;
    if (chain >= nchains) return;
    const int r = rank[chain];
    if (r < 0) return;
    const double *src = prop + (size_t)chain * D;
    double *dst = cube + (size_t)r * D;
    for (int d = lane; d < D; d += 64) dst[d] = src[d];
}

// ... one wavefront per (run, chain), lane = coordinate.  The run's base is the sum of the counts of the runs before it (at most 64 runs: one
// wave reduction); the rank becomes the GLOBAL row base + local, which the next tick reads the answers at, and the cube goes there.  Every
// run's rank array is touched by its own wavefronts only, each its own entry.  The first workgroup leaves the total in count_host[nruns].
__global__ __launch_bounds__(64) void k_park_rows_many(const PcParkRun *__restrict__ runs, int nruns, int D, const int *count, int *count_host, double *cube /* [total][D] */)
{
    const int chain = blockIdx.x, run = blockIdx.y, lane = threadIdx.x;
    const int n_l = lane < nruns ? count[lane] : 0;
    int base = lane < run ? n_l : 0, total = n_l;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { base += __shfl_xor(base, o); total += __shfl_xor(total, o); }
    if (chain == 0 && run == 0 && lane == 0) count_host[nruns] = total;
    if (run >= nruns || chain >= runs[run].nchains) return;
    int *rank = pc_as_global(runs[run].rank, runs);
    const int local = rank[chain];
    if (local < 0) return;
    const int r = base + local;
    const double *src = pc_as_global(runs[run].prop, runs) + (size_t)chain * D;
    double *dst = cube + (size_t)r * D;
    for (int d = lane; d < D; d += 64) dst[d] = src[d];
    if (lane == 0) rank[chain] = r;
}

__global__ __launch_bounds__(64) void k_live_cubes(uint32_t k0, uint32_t k1, uint32_t attempt0, int m, int D, double *cube /* [m][D] */)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= m) return;
    for (int d = lane; d < D; d += 64) cube[(size_t)i * D + d] = pc_uniform(k0, k1, PC_DOM_LIVEGEN, 0u, attempt0 + (uint32_t)i, (uint32_t)d);
}

// row j of `rows` from row idx[j] of the blocks (the layout of PcState: cube, theta at p0, phi at d0, the birth contour at b0, logL at l0)
__global__ __launch_bounds__(64) void k_live_gather(PcState S, int n, const int *idx, const double *cube, const double *theta, const double *phi,
                                                   const double *logL, double *rows /* [n][nT] */)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= n) return;
    const int i = idx[j], D = S.D, pd = S.nDer > 1 ? S.nDer : 1;
    double *row = rows + (size_t)j * S.nT;
    for (int d = lane; d < D; d += 64) { row[d] = cube[(size_t)i * D + d]; row[S.p0 + d] = theta[(size_t)i * D + d]; }
    for (int e = lane; e < S.nDer; e += 64) row[S.d0 + e] = phi[(size_t)i * pd + e];
    if (lane == 0) { row[S.b0] = S.logzero; row[S.l0] = logL[i]; }
}

extern "C" void pc_launch_park_pack(int nchains, int D, const int *need, int stride, const double *prop, int *rank, int *count, int *count_host,
                                    double *cube, hipStream_t st)
{
    hipLaunchKernelGGL(k_park_index, dim3(1), dim3(PC_PARK_THREADS), 0, st, nchains, need, stride, rank, count, count_host);
    hipLaunchKernelGGL(k_park_rows, dim3(nchains), dim3(64), 0, st, nchains, D, (const int *)rank, prop, cube);
}

extern "C" int pc_launch_park_pack_many(int nruns, const PcParkRun *runs, int max_chains, int D, int *count, int *count_host, double *cube, hipStream_t st)
{
    if (nruns < 1 || nruns > PC_PARK_MAX_RUNS || max_chains < 1) return 1;
    hipLaunchKernelGGL(k_park_index_many, dim3(nruns), dim3(PC_PARK_THREADS), 0, st, runs, count, count_host);
    hipLaunchKernelGGL(k_park_rows_many, dim3(max_chains, nruns), dim3(64), 0, st, runs, nruns, D, (const int *)count, count_host, cube);
    return 0;
}

extern "C" void pc_launch_live_cubes(const PcState *S, unsigned attempt0, int m, double *cube, hipStream_t st)
{
    hipLaunchKernelGGL(k_live_cubes, dim3(m), dim3(64), 0, st, S->k0, S->k1, (uint32_t)attempt0, m, S->D, cube);
}

extern "C" void pc_launch_live_gather(const PcState *S, int n, const int *idx, const double *cube, const double *theta, const double *phi,
                                      const double *logL, double *rows, hipStream_t st)
{
    hipLaunchKernelGGL(k_live_gather, dim3(n), dim3(64), 0, st, *S, n, idx, cube, theta, phi, logL, rows);
}
