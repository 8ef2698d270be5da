// k_tps.hip -- the Markov-bridge path sampler (mdgen_tp_sample; mdgen_amd/analysis.py tp_sample): the reference's `sample_tp`
// (mdgen/analysis.py:61-76) -- n_samples paths of length N of the chain Ta pinned at `start` and `end` -- and, with a scoring set,
// its `get_tp_likelihood(...).prod(-1)` of every path under a second chain.  The draw rule and the counter layout are stated in
// include/mdgen_amd.h; mdgen_amd/philox.py (bridge_uniform) and tests/tps_ref.py restate them in NumPy.
//   k_tp_sample   a thread owns a path.  LDS: Ta [k][k] fp64 (at most 32 KB), phi [k], and the bridge row Ba[N - t - 1] of the step
//                 every thread of the workgroup is at.  A step walks the thread's row of Ta twice: once for the total c_{k-1}, once
//                 for the first j whose cumulative sum exceeds u c_{k-1} -- the same additions in the same order, so both walks
//                 see the same sums and no per-thread array is needed.  The scoring tables are read from global memory, three
//                 values a step.
// This file is built with -ffp-contract=off (mdgen_amd/build.py EXTRA): every product below is rounded to fp64 before it is added,
// which is what lets a NumPy restatement reproduce the paths.  No atomics; a path is a function of (seed, stream, sample index).
#include "kernels.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace mdg {

// u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 of the words at counter (sample low, sample high, t, stream): 53 bits, exact, in [0, 1)
__device__ __forceinline__ double tp_uniform(uint64_t seed, uint64_t sample, uint32_t t, uint32_t stream_id) {
    const uint32_t ctr[4] = {(uint32_t)sample, (uint32_t)(sample >> 32), t, stream_id};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    return (double)(((uint64_t)(w[0] >> 5) << 26) + (uint64_t)(w[1] >> 6)) * 0x1p-53;
}

// Dynamic LDS: Ta k * k doubles, the bridge row k doubles, phi k ints.
__global__ __launch_bounds__(256) void k_tp_sample(long n_samples, int N, int k, const double* __restrict__ Ta,
                                                   const double* __restrict__ Ba, int start, int end, uint64_t seed,
                                                   uint32_t stream_id, uint64_t sample_base, int kb, const double* __restrict__ Tb,
                                                   const double* __restrict__ Bb, TpPhi phi, int* __restrict__ paths,
                                                   double* __restrict__ prob) {
    extern __shared__ __attribute__((aligned(16))) double tp_lds[];
    double* sT = tp_lds;
    double* sB = sT + k * k;
    int* sPhi = (int*)(sB + k);
    for (int i = threadIdx.x; i < k * k; i += 256) sT[i] = Ta[i];
    if (threadIdx.x == 0) {      // (constant indices: the argument is read where it lies, not copied to scratch)
#pragma unroll
        for (int i = 0; i < kTpMaxStates; ++i)
            if (i < k) sPhi[i] = phi.v[i];
    }
    __syncthreads();
    const bool score = kb > 0;
    for (long base = (long)blockIdx.x * 256; base < n_samples; base += (long)gridDim.x * 256) {
        const long s = base + threadIdx.x;
        const bool valid = s < n_samples;
        int* row = paths + (valid ? s : 0) * (long)N;
        int a = start;
        bool dead = false;       // the bridge has no weight left: the rest of the path is -1 and its prob 0
        double p = 1.0;
        if (valid) row[0] = start;
        for (int t = 1; t < N; ++t) {
            int b = end;
            if (t < N - 1) {     // (uniform: the whole workgroup stages the row of this step)
                __syncthreads();
                for (int i = threadIdx.x; i < k; i += 256) sB[i] = Ba[(long)(N - t - 1) * k + i];
                __syncthreads();
                if (valid && !dead) {
                    const double* ta = sT + a * k;
                    double total = 0.0;
                    for (int j = 0; j < k; ++j) total = total + ta[j] * sB[j];
                    if (total > 0.0) {
                        const double target = tp_uniform(seed, sample_base + (uint64_t)s, (uint32_t)t, stream_id) * total;
                        double c = 0.0;
                        int pick = -1, last_pos = 0;
                        for (int j = 0; j < k; ++j) {
                            const double w = ta[j] * sB[j];
                            c = c + w;
                            if (w > 0.0) last_pos = j;
                            if (pick < 0 && c > target) pick = j;
                        }
                        b = pick >= 0 ? pick : last_pos;
                    } else {
                        dead = true;
                    }
                }
            }
            if (valid) {
                if (dead) {
                    row[t] = -1;
                } else {
                    row[t] = b;
                    if (score) {
                        const int pa = sPhi[a], pb = sPhi[b];
                        const double f = Tb[pa * kb + pb] * Bb[(long)(N - t - 1) * kb + pb] / Bb[(long)(N - t) * kb + pa];
                        p = p * (f != f ? 0.0 : f);
                    }
                    a = b;
                }
            }
        }
        if (valid && score) prob[s] = dead ? 0.0 : p;
    }
}

void launch_tp_sample(long n_samples, int N, int k, const double* Ta, const double* Ba, int start, int end, uint64_t seed,
                      uint32_t stream_id, uint64_t sample_base, int kb, const double* Tb, const double* Bb, const TpPhi& phi,
                      int32_t* paths, double* prob, hipStream_t s) {
    const long groups = (n_samples + 255) / 256;
    const unsigned grid = (unsigned)(groups < (1l << 20) ? groups : (1l << 20));
    const size_t lds = (size_t)(k * k + k) * sizeof(double) + (size_t)k * sizeof(int);
    hipLaunchKernelGGL(k_tp_sample, dim3(grid), dim3(256), lds, s, n_samples, N, k, Ta, Ba, start, end, seed, stream_id, sample_base,
                       kb, Tb, Bb, phi, paths, prob);
}

}  // namespace mdg
