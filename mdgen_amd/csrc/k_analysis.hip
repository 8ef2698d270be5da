// k_analysis.hip -- analysis of a sampled trajectory where the sampler leaves it (mdgen_traj_dihedrals / _histograms / _acov;
// mdgen_amd/analysis.py): torsion angles of every frame, their 1-D and 2-D histograms, and the sin/cos autocovariance behind the
// reference's "decorrelation" curves (scripts/analyze_peptide_sim.py:44-96).
//   k_dihedrals      one thread per (frame, feature): the IUPAC dihedral of four atoms of the frame, fp32
//   k_torsion_hist   one workgroup per (chunk of frames, histogram): int32 counts in LDS (integer atomics), flushed to int64
//   k_sincos_prep    angles [n][NF] -> sin, cos as fp32 rows [NF][n] (evaluated in fp64, rounded once)
//   k_sincos_acov    one workgroup per (feature, lag block of 256, split of the time tiles): direct evaluation from LDS, an
//                    8 x 8 register block per thread; fp32 over 256 samples, fp64 beyond; partial sums to the workspace
//                    (the body is acov_body<2> of analysis.h, which k_tica.hip runs on one row)
//   k_acov_finish    partial sums added in split order, divided by n - k;  k_sincos_mean: the per-feature means
// No floating-point atomics anywhere: every sum has a fixed order, two calls give the same bits.
#include "analysis.h"

namespace mdg {

// ---- dihedrals ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dihedrals(const float* __restrict__ atom14, long F, long frame_floats, QuadChunk qc,
                                                   int nq, int q0, int NF, float* __restrict__ angles) {
    const long total = F * nq;
    // (vectorised across iterations, the loop's fp32 math comes out as v_pk_*_f32, which the build refuses)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long fr = i / nq;
        const int j = (int)(i - fr * nq);
        const float* base = atom14 + fr * frame_floats;
        float p[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float* q = base + (long)qc.q[j][a] * 3;
            p[a][0] = q[0];
            p[a][1] = q[1];
            p[a][2] = q[2];
        }
        float b1[3], b2[3], b3[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            b1[c] = p[1][c] - p[0][c];
            b2[c] = p[2][c] - p[1][c];
            b3[c] = p[3][c] - p[2][c];
        }
        const float c1[3] = {b2[1] * b3[2] - b2[2] * b3[1], b2[2] * b3[0] - b2[0] * b3[2], b2[0] * b3[1] - b2[1] * b3[0]};
        const float c2[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
        const float nb2 = sqrtf(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]);
        const float y = nb2 * (b1[0] * c1[0] + b1[1] * c1[1] + b1[2] * c1[2]);
        const float x = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2];
        // coincident or collinear atoms: 0 whatever the signs of the two zeros (atan2f(+-0, -0) is +-pi)
        angles[fr * NF + q0 + j] = (x == 0.f && y == 0.f) ? 0.f : atan2f(y, x);
    }
}

void launch_dihedrals(long F, int L, int NF, const float* atom14, const int32_t* quad_host, float* angles, hipStream_t s) {
    for (int q0 = 0; q0 < NF; q0 += kQuadChunk) {
        QuadChunk qc;
        const int nq = NF - q0 < kQuadChunk ? NF - q0 : kQuadChunk;
        for (int j = 0; j < nq; ++j)
            for (int a = 0; a < 4; ++a) qc.q[j][a] = quad_host[(long)(q0 + j) * 4 + a];
        const long want = (F * nq + 255) / 256;
        const unsigned grid = (unsigned)(want < (1l << 20) ? want : (1l << 20));
        hipLaunchKernelGGL(k_dihedrals, dim3(grid), dim3(256), 0, s, atom14, F, (long)L * 42, qc, nq, q0, NF, angles);
    }
}

// ---- histograms -----------------------------------------------------------------------------------------------------
// blockIdx.y: histogram unit -- u < n1: the 1-D histogram of feature u; else pair u - n1 of this launch's chunk.
// blockIdx.x: frames [x * chunk, (x + 1) * chunk).  Dynamic LDS: max(bins1, bins2 * bins2) ints.
__global__ __launch_bounds__(256) void k_torsion_hist(const float* __restrict__ angles, long F, int NF, long chunk, int n1, int bins1,
                                                      const double* __restrict__ edges1, PairChunk pc, int pair0, int bins2,
                                                      const double* __restrict__ edges2, unsigned long long* __restrict__ hist1,
                                                      unsigned long long* __restrict__ hist2,
                                                      unsigned long long* __restrict__ dropped) {
    extern __shared__ int cnt[];
    const int u = blockIdx.y;
    const bool one = u < n1;
    const int nb = one ? bins1 : bins2 * bins2;
    for (int i = threadIdx.x; i < nb; i += 256) cnt[i] = 0;
    __syncthreads();
    const long f0 = (long)blockIdx.x * chunk;
    const long f1 = f0 + chunk < F ? f0 + chunk : F;
    int drop = 0;
    if (one) {
        for (long fr = f0 + threadIdx.x; fr < f1; fr += 256) {
            const int b = hist_bin((double)angles[fr * NF + u], edges1, bins1);
            if (b < 0)
                ++drop;
            else
                atomicAdd(&cnt[b], 1);
        }
    } else {
        const int fx = pc.p[u - n1][0], fy = pc.p[u - n1][1];
        for (long fr = f0 + threadIdx.x; fr < f1; fr += 256) {
            const int bx = hist_bin((double)angles[fr * NF + fx], edges2, bins2);
            const int by = hist_bin((double)angles[fr * NF + fy], edges2, bins2);
            if (bx < 0 || by < 0)
                ++drop;
            else
                atomicAdd(&cnt[bx * bins2 + by], 1);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) drop += __shfl_xor(drop, o);
    __syncthreads();
    unsigned long long* out = one ? hist1 + (long)u * bins1 : hist2 + (long)(pair0 + u - n1) * nb;
    for (int i = threadIdx.x; i < nb; i += 256)
        if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
    if ((threadIdx.x & 63) == 0 && drop) atomicAdd(&dropped[one ? u : NF + pair0 + u - n1], (unsigned long long)drop);
}

// hist1, hist2 and dropped are zero on entry (the caller's memsets on `s`)
void launch_torsion_hist(long F, int NF, const float* angles, int bins1, const double* edges1, int P, const int32_t* pairs_host,
                         int bins2, const double* edges2, int64_t* hist1, int64_t* hist2, int64_t* dropped, hipStream_t s) {
    long chunk = 4096;
    if ((F + chunk - 1) / chunk > (1l << 20)) chunk = (F + (1l << 20) - 1) >> 20;
    const unsigned gx = (unsigned)((F + chunk - 1) / chunk);
    int n1 = NF;
    for (int p0 = 0; p0 < P || n1 > 0; p0 += kPairChunk) {
        PairChunk pc;
        int np = P - p0 < kPairChunk ? P - p0 : kPairChunk;
        if (np < 0) np = 0;
        for (int j = 0; j < np; ++j) {
            pc.p[j][0] = pairs_host[(long)(p0 + j) * 2];
            pc.p[j][1] = pairs_host[(long)(p0 + j) * 2 + 1];
        }
        const int nb1 = n1 ? bins1 : 0, nb2 = np ? bins2 * bins2 : 0;
        const int nb = nb1 > nb2 ? nb1 : nb2;
        hipLaunchKernelGGL(k_torsion_hist, dim3(gx, (unsigned)(n1 + np)), dim3(256), (size_t)nb * sizeof(int), s, angles, F, NF, chunk,
                           n1, bins1, edges1, pc, p0, bins2, edges2, (unsigned long long*)hist1, (unsigned long long*)hist2,
                           (unsigned long long*)dropped);
        n1 = 0;
    }
}

// ---- sin/cos autocovariance -----------------------------------------------------------------------------------------
constexpr long kAcTargetGroups = 2048;          // workgroups wanted on the chip (8 a CU)
constexpr int kAcMaxSplits = 64;

static long ac_lag_blocks(long K) { return (K + 1 + kAcLB - 1) / kAcLB; }

int acov_splits(long n, int NF, long K) {
    const long base = (long)NF * ac_lag_blocks(K), tiles = (n + kAcTT - 1) / kAcTT;
    long S = base > 0 ? (kAcTargetGroups + base - 1) / base : 1;
    S = S > tiles ? tiles : S;
    S = S > kAcMaxSplits ? kAcMaxSplits : S;
    return (int)(S < 1 ? 1 : S);
}

// partial sums [NF][S][K + 1] fp64, then the sin rows and the cos rows [NF][n] fp32
size_t acov_workspace_bytes(long n, int NF, long K) {
    return (size_t)NF * acov_splits(n, NF, K) * (size_t)(K + 1) * sizeof(double) + 2 * (size_t)NF * (size_t)n * sizeof(float);
}

long acov_groups(long n, int NF, long K) { return (long)NF * acov_splits(n, NF, K) * ac_lag_blocks(K); }

__global__ __launch_bounds__(256) void k_sincos_prep(const float* __restrict__ angles, long n, int NF, float* __restrict__ S,
                                                     float* __restrict__ Cc) {
    const long total = n * NF;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = i / NF;
        const int f = (int)(i - t * NF);
        double sn, cs;
        sincos((double)angles[i], &sn, &cs);
        S[(long)f * n + t] = (float)sn;
        Cc[(long)f * n + t] = (float)cs;
    }
}

__global__ __launch_bounds__(256) void k_sincos_mean(const float* __restrict__ S, const float* __restrict__ Cc, long n,
                                                     double* __restrict__ mean_sin, double* __restrict__ mean_cos) {
    __shared__ double rs[256], rc[256];
    const int f = blockIdx.x;
    double a = 0, b = 0;
    for (long t = threadIdx.x; t < n; t += 256) {
        a += (double)S[(long)f * n + t];
        b += (double)Cc[(long)f * n + t];
    }
    rs[threadIdx.x] = a;
    rc[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            rs[threadIdx.x] += rs[threadIdx.x + o];
            rc[threadIdx.x] += rc[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mean_sin[f] = rs[0] / (double)n;
        mean_cos[f] = rc[0] / (double)n;
    }
}

// acov_body<2> (analysis.h): the sin row and the cos row of feature f, their products summed
__global__ __launch_bounds__(256) void k_sincos_acov(const float* __restrict__ S, const float* __restrict__ Cc, long n, long K,
                                                     int splits, int lag_blocks, double* __restrict__ partial) {
    acov_body<2>(S, Cc, n, K, splits, lag_blocks, partial);
}

__global__ __launch_bounds__(256) void k_acov_finish(const double* __restrict__ partial, long n, long K, int NF, int splits,
                                                     double* __restrict__ acov) {
    const long total = (long)NF * (K + 1);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long f = i / (K + 1), k = i - f * (K + 1);
        double sum = 0.0;
        for (int sp = 0; sp < splits; ++sp) sum += partial[(f * splits + sp) * (K + 1) + k];
        acov[i] = sum / (double)(n - k);
    }
}

void launch_acov_finish(const double* partial, long n, long K, int NF, int splits, double* acov, hipStream_t s) {
    const long fin = ((long)NF * (K + 1) + 255) / 256;
    hipLaunchKernelGGL(k_acov_finish, dim3((unsigned)(fin < (1l << 20) ? fin : (1l << 20))), dim3(256), 0, s, partial, n, K, NF, splits,
                       acov);
}

void launch_sincos_acov(long n, int NF, long K, const float* angles, double* acov, double* mean_sin, double* mean_cos, void* ws,
                        hipStream_t s) {
    const int splits = acov_splits(n, NF, K);
    const int lag_blocks = (int)ac_lag_blocks(K);
    double* partial = (double*)ws;
    float* S = (float*)(partial + (size_t)NF * splits * (size_t)(K + 1));
    float* Cc = S + (size_t)NF * (size_t)n;
    const long want = (n * NF + 255) / 256;
    hipLaunchKernelGGL(k_sincos_prep, dim3((unsigned)(want < (1l << 20) ? want : (1l << 20))), dim3(256), 0, s, angles, n, NF, S, Cc);
    hipLaunchKernelGGL(k_sincos_mean, dim3((unsigned)NF), dim3(256), 0, s, S, Cc, n, mean_sin, mean_cos);
    hipLaunchKernelGGL(k_sincos_acov, dim3((unsigned)acov_groups(n, NF, K)), dim3(256), 0, s, S, Cc, n, K, splits, lag_blocks, partial);
    launch_acov_finish(partial, n, K, NF, splits, acov, s);
}

}  // namespace mdg
