// k_tica.hip -- the device side of tICA on a trajectory's torsion angles (mdgen_traj_lagged_moments / _project / _series_acov /
// _histograms_xy; mdgen_amd/analysis.py tica_fit, tica_transform): everything that scales with the trajectory length.  The D x D
// eigenproblem (D = 2 NF <= 128) is the host's.
//   k_feat_prep       angles [n][NF] -> features [n][D] fp32, x[2j] = cos a_j, x[2j + 1] = sin a_j (evaluated in fp64, rounded once)
//   k_moments         one workgroup per (split of the frames, 64 x 64 tile of the matrices): 64 frames of X and of Y staged in LDS
//                     feed X'X, Y'Y and X'Y, a 4 x 4 register block of each per thread; fp32 over 64 frames, fp64 beyond; the column
//                     sums of X and Y in fp64 on the side
//   k_moments_finish  partial sums added in a fixed order of the splits
//   k_project         out[t][c] = sum_j (x_t[j] - mean[j]) W[j][c]: 64 frames' centred features in LDS, fp32 FMAs with j ascending
//   k_series_prep / k_series_mean / k_series_acov    a plain series through acov_body<1> (analysis.h)
//   k_hist_xy         k_torsion_hist's pair branch with an edge table per pair and axis
// No floating-point atomics anywhere: every sum has a fixed order, two calls give the same bits.
#include "analysis.h"

namespace mdg {

// ---- lagged moments -------------------------------------------------------------------------------------------------
constexpr int kMoT = 64;                  // frames staged at a time: the length of an fp32 partial sum (the rule allows 256)
constexpr int kMoTile = 64;               // features of a tile side (4 per thread, 16 x 16 threads)
constexpr long kMoTargetGroups = 512;     // workgroups wanted on the chip: two a CU, what 200 registers a thread admit
constexpr int kMoMaxSplits = 512;
constexpr int kMoFinE = 64, kMoFinQ = 4;  // k_moments_finish: elements a workgroup, split groups

static int mo_tiles(int NF) { return (2 * NF + kMoTile - 1) / kMoTile; }

static int mo_splits(long m, int NF) {
    const long runs = (m + kMoT - 1) / kMoT, per = (long)mo_tiles(NF) * mo_tiles(NF);
    long S = (kMoTargetGroups + per - 1) / per;
    S = S > runs ? runs : S;
    S = S > kMoMaxSplits ? kMoMaxSplits : S;
    return (int)(S < 1 ? 1 : S);
}

// frames of a split: a multiple of kMoT; splits * chunk >= m
static long mo_chunk(long m, int S) {
    const long runs = (m + kMoT - 1) / kMoT;
    return (runs + S - 1) / S * kMoT;
}

// partial matrices [S][3][D][D] fp64, partial sums [S][2][D] fp64, then the features [n][D] fp32
size_t moments_workspace_bytes(long n, int NF, long lag) {
    const size_t D = 2 * (size_t)NF, S = (size_t)mo_splits(n - lag, NF);
    return S * (3 * D * D + 2 * D) * sizeof(double) + (size_t)n * D * sizeof(float);
}

__global__ __launch_bounds__(256) void k_feat_prep(const float* __restrict__ angles, long n, int NF, float* __restrict__ feat) {
    const long total = n * NF;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        double sn, cs;
        sincos((double)angles[i], &sn, &cs);
        feat[2 * i] = (float)cs;       // i = t * NF + j: float 2 i is feature 2 j of frame t
        feat[2 * i + 1] = (float)sn;
    }
}

// acc[r][c] += a[r] * b[c]
__device__ __forceinline__ void mo_outer(const float4& a4, const float4& b4, float (&acc)[4][4]) {
    const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
}

__device__ __forceinline__ void mo_flush(float (&acc)[4][4], double (&acc64)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc64[r][c] += (double)acc[r][c];
            acc[r][c] = 0.f;
        }
}

// blockIdx.x: split (frames [x * chunk, (x + 1) * chunk) of the m lagged pairs);  blockIdx.y: tile (row tile ti, column tile tj) of
// the D x D matrices.  With X = x[0 .. m), Y = x[lag .. n): 64 frames of X and of Y, feature tiles ti and tj, are staged once and
// feed the tile of X'X, of Y'Y and of X'Y (dynamic LDS: two 16 KB tiles where ti == tj -- always, for D <= 64 -- else four).  Rows
// beyond the split and columns beyond D are staged as zeros: their products vanish without a branch.  The three matrices see the
// same operations in the same order: at lag 0, where Y = X, they are equal to the bit.  Column tile 0 also adds up the columns of
// its X and Y row tiles (sx, sy), in fp64.
__global__ __launch_bounds__(256) void k_moments(const float* __restrict__ feat, long m, long lag, int D, long chunk, int tiles,
                                                 double* __restrict__ partial, double* __restrict__ psum) {
    extern __shared__ __attribute__((aligned(16))) float mo_lds[];
    typedef float Tile[kMoT][kMoTile];
    const int i0 = (int)(blockIdx.y / tiles) * kMoTile, j0 = (int)(blockIdx.y % tiles) * kMoTile;
    const bool diag = i0 == j0;
    Tile& Xi = *(Tile*)mo_lds;
    Tile& Yi = *(Tile*)(mo_lds + kMoT * kMoTile);
    Tile& Xj = diag ? Xi : *(Tile*)(mo_lds + 2 * kMoT * kMoTile);
    Tile& Yj = diag ? Yi : *(Tile*)(mo_lds + 3 * kMoT * kMoTile);
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
    const long t_begin = (long)blockIdx.x * chunk;
    const long t_end = t_begin + chunk < m ? t_begin + chunk : m;
    double cxx64[4][4], cyy64[4][4], cxy64[4][4], colsum = 0.0;
    float cxx[4][4], cyy[4][4], cxy[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            cxx64[r][c] = cyy64[r][c] = cxy64[r][c] = 0.0;
            cxx[r][c] = cyy[r][c] = cxy[r][c] = 0.f;
        }
    for (long t0 = t_begin; t0 < t_end; t0 += kMoT) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < kMoT * kMoTile; idx += 256) {
            const int tt = idx >> 6, ii = idx & 63;
            const long t = t0 + tt;
            const bool in_i = t < t_end && i0 + ii < D;
            Xi[tt][ii] = in_i ? feat[t * D + i0 + ii] : 0.f;
            Yi[tt][ii] = in_i ? feat[(t + lag) * D + i0 + ii] : 0.f;
            if (!diag) {
                const bool in_j = t < t_end && j0 + ii < D;
                Xj[tt][ii] = in_j ? feat[t * D + j0 + ii] : 0.f;
                Yj[tt][ii] = in_j ? feat[(t + lag) * D + j0 + ii] : 0.f;
            }
        }
        __syncthreads();
        if (j0 == 0 && threadIdx.x < 2 * kMoTile) {   // waves 0 and 1: column threadIdx.x & 63 of Xi / of Yi, frames ascending
            const Tile& src = threadIdx.x < kMoTile ? Xi : Yi;
            for (int tt = 0; tt < kMoT; ++tt) colsum += (double)src[tt][threadIdx.x & (kMoTile - 1)];
        }
#pragma unroll 2
        for (int tt = 0; tt < kMoT; ++tt) {
            const float4 xa = *(const float4*)&Xi[tt][tr * 4], ya = *(const float4*)&Yi[tt][tr * 4];
            const float4 xb = *(const float4*)&Xj[tt][tc * 4], yb = *(const float4*)&Yj[tt][tc * 4];
            mo_outer(xa, xb, cxx);
            mo_outer(ya, yb, cyy);
            mo_outer(xa, yb, cxy);
        }
        mo_flush(cxx, cxx64);
        mo_flush(cyy, cyy64);
        mo_flush(cxy, cxy64);
    }
    double* out = partial + (size_t)blockIdx.x * 3 * (size_t)D * D;   // every (split, matrix, i, j) is written
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + tr * 4 + r, j = j0 + tc * 4 + c;
            if (i < D && j < D) {
                out[(size_t)i * D + j] = cxx64[r][c];
                out[(size_t)D * D + (size_t)i * D + j] = cyy64[r][c];
                out[2 * (size_t)D * D + (size_t)i * D + j] = cxy64[r][c];
            }
        }
    const int col = i0 + (threadIdx.x & (kMoTile - 1));
    if (j0 == 0 && threadIdx.x < 2 * kMoTile && col < D)
        psum[((size_t)blockIdx.x * 2 + (threadIdx.x >> 6)) * D + col] = colsum;
}

// Workgroup: kMoFinE consecutive elements of (cxx, cyy, cxy, sx, sy); thread (q, e) adds splits q, q + 4, ... in ascending order,
// the four sums meet in LDS and are added in the order of q.
__global__ __launch_bounds__(256) void k_moments_finish(const double* __restrict__ partial, const double* __restrict__ psum, int D,
                                                        int splits, double* __restrict__ sx, double* __restrict__ sy,
                                                        double* __restrict__ cxx, double* __restrict__ cyy, double* __restrict__ cxy) {
    __shared__ double red[kMoFinQ][kMoFinE];
    const long DD = (long)D * D, total = 3 * DD + 2 * D;
    const int el = threadIdx.x & (kMoFinE - 1), q = threadIdx.x / kMoFinE;
    const long e = (long)blockIdx.x * kMoFinE + el;
    double sum = 0.0;
    if (e < total) {
        const bool mat = e < 3 * DD;
        const double* src = mat ? partial + e : psum + (e - 3 * DD);
        const size_t stride = mat ? 3 * (size_t)DD : 2 * (size_t)D;
#pragma unroll 8
        for (int sp = q; sp < splits; sp += kMoFinQ) sum += src[(size_t)sp * stride];
    }
    red[q][el] = sum;
    __syncthreads();
    if (q == 0 && e < total) {
        sum = ((red[0][el] + red[1][el]) + red[2][el]) + red[3][el];
        if (e < 3 * DD) {
            const long which = e / DD, r = e - which * DD;
            (which == 0 ? cxx : which == 1 ? cyy : cxy)[r] = sum;
        } else {
            const long e2 = e - 3 * DD;
            if (e2 < D)
                sx[e2] = sum;
            else
                sy[e2 - D] = sum;
        }
    }
}

void launch_lagged_moments(long n, int NF, long lag, const float* angles, double* sx, double* sy, double* cxx, double* cyy, double* cxy,
                           void* ws, hipStream_t s) {
    const int D = 2 * NF, tiles = mo_tiles(NF);
    const long m = n - lag;
    const int splits = mo_splits(m, NF);
    const long chunk = mo_chunk(m, splits);
    double* partial = (double*)ws;
    double* psum = partial + (size_t)splits * 3 * D * D;
    float* feat = (float*)(psum + (size_t)splits * 2 * D);
    const long want = (n * NF + 255) / 256;
    hipLaunchKernelGGL(k_feat_prep, dim3((unsigned)(want < (1l << 20) ? want : (1l << 20))), dim3(256), 0, s, angles, n, NF, feat);
    const size_t lds = (size_t)(tiles == 1 ? 2 : 4) * kMoT * kMoTile * sizeof(float);
    hipLaunchKernelGGL(k_moments, dim3((unsigned)splits, (unsigned)(tiles * tiles)), dim3(256), lds, s, feat, m, lag, D, chunk, tiles,
                       partial, psum);
    const long fin = (3l * D * D + 2 * D + kMoFinE - 1) / kMoFinE;
    hipLaunchKernelGGL(k_moments_finish, dim3((unsigned)fin), dim3(256), 0, s, partial, psum, D, splits, sx, sy, cxx, cyy, cxy);
}

// ---- projection -----------------------------------------------------------------------------------------------------
constexpr int kPrT = 64;   // frames of a block.  Dynamic LDS: kPrT * D floats.

__global__ __launch_bounds__(256) void k_project(const float* __restrict__ angles, long n, int NF, int d, const float* __restrict__ mean,
                                                 const float* __restrict__ W, float* __restrict__ out) {
    extern __shared__ float xs[];
    const int D = 2 * NF;
    const long blocks = (n + kPrT - 1) / kPrT;
    for (long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const long t0 = blk * kPrT;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kPrT * NF; idx += 256) {
            const int tt = idx / NF, j = idx - tt * NF;
            if (t0 + tt < n) {
                double sn, cs;
                sincos((double)angles[(t0 + tt) * NF + j], &sn, &cs);
                xs[tt * D + 2 * j] = (float)cs - mean[2 * j];
                xs[tt * D + 2 * j + 1] = (float)sn - mean[2 * j + 1];
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < kPrT * d; idx += 256) {
            const int tt = idx / d, c = idx - tt * d;
            if (t0 + tt < n) {
                float acc = 0.f;
                for (int j = 0; j < D; ++j) acc = fmaf(xs[tt * D + j], W[j * d + c], acc);
                out[(t0 + tt) * d + c] = acc;
            }
        }
    }
}

void launch_project(long n, int NF, int d, const float* angles, const float* mean, const float* W, float* out, hipStream_t s) {
    const long blocks = (n + kPrT - 1) / kPrT;
    hipLaunchKernelGGL(k_project, dim3((unsigned)(blocks < (1l << 20) ? blocks : (1l << 20))), dim3(256),
                       (size_t)kPrT * 2 * NF * sizeof(float), s, angles, n, NF, d, mean, W, out);
}

// ---- autocovariance of a plain series -------------------------------------------------------------------------------
// partial sums [NS][splits][K + 1] fp64 (mdgen_traj_acov's splits), then the rows [NS][n] fp32
size_t series_acov_workspace_bytes(long n, int NS, long K) {
    return (size_t)NS * acov_splits(n, NS, K) * (size_t)(K + 1) * sizeof(double) + (size_t)NS * (size_t)n * sizeof(float);
}

__global__ __launch_bounds__(256) void k_series_prep(const float* __restrict__ x, long n, int NS, float* __restrict__ rows) {
    const long total = n * NS;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = i / NS;
        const int f = (int)(i - t * NS);
        rows[(long)f * n + t] = x[i];
    }
}

__global__ __launch_bounds__(256) void k_series_mean(const float* __restrict__ rows, long n, double* __restrict__ mean) {
    __shared__ double red[256];
    const int f = blockIdx.x;
    double a = 0;
    for (long t = threadIdx.x; t < n; t += 256) a += (double)rows[(long)f * n + t];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[f] = red[0] / (double)n;
}

__global__ __launch_bounds__(256) void k_series_acov(const float* __restrict__ rows, long n, long K, int splits, int lag_blocks,
                                                     double* __restrict__ partial) {
    acov_body<1>(rows, nullptr, n, K, splits, lag_blocks, partial);
}

void launch_series_acov(long n, int NS, long K, const float* x, double* acov, double* mean, void* ws, hipStream_t s) {
    const int splits = acov_splits(n, NS, K);
    const int lag_blocks = (int)((K + 1 + kAcLB - 1) / kAcLB);
    double* partial = (double*)ws;
    float* rows = (float*)(partial + (size_t)NS * splits * (size_t)(K + 1));
    const long want = (n * NS + 255) / 256;
    hipLaunchKernelGGL(k_series_prep, dim3((unsigned)(want < (1l << 20) ? want : (1l << 20))), dim3(256), 0, s, x, n, NS, rows);
    hipLaunchKernelGGL(k_series_mean, dim3((unsigned)NS), dim3(256), 0, s, rows, n, mean);
    hipLaunchKernelGGL(k_series_acov, dim3((unsigned)acov_groups(n, NS, K)), dim3(256), 0, s, rows, n, K, splits, lag_blocks, partial);
    launch_acov_finish(partial, n, K, NS, splits, acov, s);
}

// ---- 2-D histograms, an edge table per pair and axis ----------------------------------------------------------------
// blockIdx.y: pair of this launch's chunk;  blockIdx.x: frames [x * chunk, (x + 1) * chunk).  Dynamic LDS: bins * bins ints.
__global__ __launch_bounds__(256) void k_hist_xy(const float* __restrict__ values, long F, int NC, long chunk, PairChunk pc, int pair0,
                                                 int bins, const double* __restrict__ edges_x, const double* __restrict__ edges_y,
                                                 unsigned long long* __restrict__ hist2, unsigned long long* __restrict__ dropped) {
    extern __shared__ int cnt[];
    const int u = blockIdx.y, p = pair0 + u, nb = bins * bins;
    for (int i = threadIdx.x; i < nb; i += 256) cnt[i] = 0;
    __syncthreads();
    const double* ex = edges_x + (long)p * (bins + 1);
    const double* ey = edges_y + (long)p * (bins + 1);
    const long f0 = (long)blockIdx.x * chunk;
    const long f1 = f0 + chunk < F ? f0 + chunk : F;
    const int cx = pc.p[u][0], cy = pc.p[u][1];
    int drop = 0;
    for (long fr = f0 + threadIdx.x; fr < f1; fr += 256) {
        const int bx = hist_bin((double)values[fr * NC + cx], ex, bins);
        const int by = hist_bin((double)values[fr * NC + cy], ey, bins);
        if (bx < 0 || by < 0)
            ++drop;
        else
            atomicAdd(&cnt[bx * bins + by], 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) drop += __shfl_xor(drop, o);
    __syncthreads();
    unsigned long long* out = hist2 + (long)p * nb;
    for (int i = threadIdx.x; i < nb; i += 256)
        if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
    if ((threadIdx.x & 63) == 0 && drop) atomicAdd(&dropped[p], (unsigned long long)drop);
}

void launch_hist_xy(long F, int NC, const float* values, int P, const int32_t* pairs_host, int bins, const double* edges_x,
                    const double* edges_y, int64_t* hist2, int64_t* dropped, hipStream_t s) {
    long chunk = 4096;
    if ((F + chunk - 1) / chunk > (1l << 20)) chunk = (F + (1l << 20) - 1) >> 20;
    const unsigned gx = (unsigned)((F + chunk - 1) / chunk);
    for (int p0 = 0; p0 < P; p0 += kPairChunk) {
        PairChunk pc;
        const int np = P - p0 < kPairChunk ? P - p0 : kPairChunk;
        for (int j = 0; j < np; ++j) {
            pc.p[j][0] = pairs_host[(long)(p0 + j) * 2];
            pc.p[j][1] = pairs_host[(long)(p0 + j) * 2 + 1];
        }
        hipLaunchKernelGGL(k_hist_xy, dim3(gx, (unsigned)np), dim3(256), (size_t)bins * bins * sizeof(int), s, values, F, NC, chunk, pc, p0,
                           bins, edges_x, edges_y, (unsigned long long*)hist2, (unsigned long long*)dropped);
    }
}

}  // namespace mdg
