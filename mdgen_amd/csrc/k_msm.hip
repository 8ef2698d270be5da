// k_msm.hip -- the device side of the k-means / Markov-state-model analysis (mdgen_traj_kmeans_assign / _kmeans_step / _kmeans_pp /
// _count_matrix; mdgen_amd/analysis.py kmeans_fit, count_matrix): everything that scales with the trajectory length.  The k x k
// estimators (connected set, reversible MLE, PCCA+; k <= 256) are the host's: mdgen_amd/msm.py.
//   k_km_assign     a thread owns a point; the centres pass through LDS in tiles of at most 32 KB and are read as broadcasts; kKmCT
//                   distances a thread at a time, each sum_j (x_j - c_j)^2 with fp32 FMAs over j ascending; ties to the lowest index.
//                   With `cost_partial`: the workgroup's fp64 sum of its points' distances, in a fixed order
//   k_km_accum      one workgroup per (split of the points, tile of the dimensions): a thread owns one (sub-chunk, dimension) column
//                   of LDS fp64 accumulators [cluster] and walks its sub-chunk's points in order; the sub-chunks are added in order
//   k_km_finish     partial sums and counts added in a fixed order of the splits; centres = fp32(sum / count), an empty cluster's kept
//   k_km_update     cost partials added in a fixed order; cost[1] <- cost[0] <- cost; the done flag and the step counter
//   k_pp_init / k_pp_update / k_pp_select      k-means++: mind2 and its fp64 sums per 256 points; one workgroup finds the index
//   k_count_matrix  sliding-window transition counts: integer atomics, per workgroup in LDS where k * k ints fit 48 KB
// No floating-point atomics anywhere: every sum has a fixed order, two calls give the same bits.  The kernels of a Lloyd step read
// state[0] (the done flag) and return at once when it is set; only k_km_update, the last of a step, writes it.
#include "analysis.h"

namespace mdg {

constexpr int kKmCenterFloats = 8192;   // floats of the LDS centre tile (32 KB): at d = 128 that is 64 centres
constexpr int kKmCT = 8;                // centres a thread measures at a time
constexpr int kKmMaxGroups = 1024;      // workgroups of k_km_assign, and the number of cost partials
constexpr int kKmAccDoubles = 4096;     // fp64 accumulators of a k_km_accum workgroup (32 KB) ...
constexpr int kKmAccInts = 4096;        // ... and its counters (16 KB)
constexpr long kKmPartialDoubles = 1l << 21;   // 16 MB of partial sums at the most
constexpr int kKmMaxSplits = 1024;
constexpr int kKmAB = 8;                // points whose assignment and value a k_km_accum thread loads ahead of their LDS updates
constexpr int kPpSeg = 256;             // points of a k-means++ segment

static int km_groups(long n) {
    const long g = (n + 255) / 256;
    return (int)(g < kKmMaxGroups ? g : kKmMaxGroups);
}

static int km_row(int d) { return (d + 3) & ~3; }   // floats of a centre's LDS row: the pad holds zeros

static int km_center_tile(int d, int k) {
    const int kt = kKmCenterFloats / km_row(d);   // >= 64
    return kt < k ? kt : k;
}

// k_km_accum's shape: DT dimensions of a tile, Q sub-chunks a workgroup (Q * DT <= 256 threads, Q * k * DT <= kKmAccDoubles,
// Q * k <= kKmAccInts), S splits of the points
struct KmAccShape {
    int DT, Q, S, tiles;
    long chunk;
};

static KmAccShape km_acc_shape(long n, int d, int k) {
    KmAccShape a;
    a.DT = kKmAccDoubles / k < d ? kKmAccDoubles / k : d;   // k <= 256: DT >= 16 or d
    a.Q = 256 / a.DT;
    if (a.Q > kKmAccDoubles / (k * a.DT)) a.Q = kKmAccDoubles / (k * a.DT);
    if (a.Q > kKmAccInts / k) a.Q = kKmAccInts / k;
    if (a.Q < 1) a.Q = 1;
    a.tiles = (d + a.DT - 1) / a.DT;
    long S = kKmMaxSplits / a.tiles;
    const long cap = kKmPartialDoubles / ((long)k * d), runs = (n + 255) / 256;
    S = S > cap ? cap : S;
    S = S > runs ? runs : S;
    a.S = (int)(S < 1 ? 1 : S);
    a.chunk = (n + a.S - 1) / a.S;
    a.S = (int)((n + a.chunk - 1) / a.chunk);   // no empty split
    return a;
}

// cost partials [kKmMaxGroups] fp64, partial sums [S][k][d] fp64, partial counts [S][k] int64
size_t kmeans_step_workspace_bytes(long n, int d, int k) {
    const KmAccShape a = km_acc_shape(n, d, k);
    return (size_t)kKmMaxGroups * sizeof(double) + (size_t)a.S * k * d * sizeof(double) + (size_t)a.S * k * sizeof(long long);
}

// segment sums [ceil(n / kPpSeg)] fp64
size_t kmeans_pp_workspace_bytes(long n) { return (size_t)((n + kPpSeg - 1) / kPpSeg) * sizeof(double); }

// ---- assignment -----------------------------------------------------------------------------------------------------
// The nearest of the kt centres cs[kt][dp] (LDS; dp = d rounded up to 4, the pad zero) to the row xr: distances in groups of kKmCT,
// each its own chain of FMAs over j ascending; four j at a time, the centres' as one 16-byte broadcast read.  A padded term is
// fma(0, 0, acc) = acc.  `<` in ascending index keeps the lowest index on ties.  A group's slots beyond kt repeat centre kt - 1
// and are ignored.
__device__ __forceinline__ void km_nearest(const float* __restrict__ xr, const float* cs, int kt, int d, int dp, int c_base,
                                           float& best, int& arg) {
    for (int c0 = 0; c0 < kt; c0 += kKmCT) {
        float acc[kKmCT];
        int off[kKmCT];
#pragma unroll
        for (int cc = 0; cc < kKmCT; ++cc) {
            acc[cc] = 0.f;
            off[cc] = (c0 + cc < kt ? c0 + cc : kt - 1) * dp;
        }
        for (int j = 0; j < dp; j += 4) {
            float xv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = j + e < d ? xr[j + e] : 0.f;
#pragma unroll
            for (int cc = 0; cc < kKmCT; ++cc) {
                const float4 c4 = *(const float4*)&cs[off[cc] + j];
                const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float diff = xv[e] - cv[e];
                    acc[cc] = fmaf(diff, diff, acc[cc]);
                }
            }
        }
#pragma unroll
        for (int cc = 0; cc < kKmCT; ++cc)
            if (c0 + cc < kt && acc[cc] < best) {
                best = acc[cc];
                arg = c_base + c0 + cc;
            }
    }
}

// sum of red[0 .. 256) in a fixed tree; the result in every thread
__device__ __forceinline__ double km_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// Workgroup b: points b * 256 + threadIdx.x, then a grid's stride further on.  Dynamic LDS: kt_max * km_row(d) floats.
__global__ __launch_bounds__(256) void k_km_assign(const float* __restrict__ x, long n, int d, int k, int kt_max,
                                                   const float* __restrict__ centers, const int* __restrict__ state,
                                                   int* __restrict__ assign, float* __restrict__ dist2,
                                                   double* __restrict__ cost_partial) {
    extern __shared__ __attribute__((aligned(16))) float km_cs[];
    __shared__ double red[256];
    if (state && state[0]) return;
    const bool one_tile = kt_max >= k;
    const int dp = (d + 3) & ~3;
    bool loaded = false;
    double cost = 0.0;
    for (long base = (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {
        const long t = base + threadIdx.x;
        const bool valid = t < n;
        float best = __builtin_inff();
        int arg = 0;
        for (int c_base = 0; c_base < k; c_base += kt_max) {
            const int kt = k - c_base < kt_max ? k - c_base : kt_max;
            if (!(one_tile && loaded)) {
                __syncthreads();
                for (int i = threadIdx.x; i < kt * dp; i += 256) {
                    const int c = i / dp, j = i - c * dp;
                    km_cs[i] = j < d ? centers[(long)(c_base + c) * d + j] : 0.f;
                }
                __syncthreads();
                loaded = true;
            }
            if (valid) km_nearest(x + t * d, km_cs, kt, d, dp, c_base, best, arg);
        }
        if (valid) {
            assign[t] = arg;
            if (dist2) dist2[t] = best;
            cost += (double)best;
        }
    }
    if (cost_partial) {
        const double s = km_block_sum(cost, red);
        if (threadIdx.x == 0) cost_partial[blockIdx.x] = s;
    }
}

void launch_kmeans_assign(long n, int d, int k, const float* x, const float* centers, int32_t* assign, float* dist2, hipStream_t s) {
    const int kt = km_center_tile(d, k);
    hipLaunchKernelGGL(k_km_assign, dim3((unsigned)km_groups(n)), dim3(256), (size_t)kt * km_row(d) * sizeof(float), s, x, n, d, k, kt,
                       centers, (const int*)nullptr, assign, dist2, (double*)nullptr);
}

// ---- one Lloyd step -------------------------------------------------------------------------------------------------
// blockIdx.x: split (points [x * chunk, (x + 1) * chunk));  blockIdx.y: dimensions [y * DT, (y + 1) * DT).  Thread (q, jj),
// q = threadIdx.x / DT < Q: sub-chunk q of the split, dimension y * DT + jj; the workgroup has Q * DT threads rounded up to whole
// waves.  Dynamic LDS: acc fp64 [Q][k][DT], then cnt int [Q][k].  A thread's chain is load -> LDS read-add-write per point: the
// loads of kKmAB points are issued together, their updates follow in the points' order.
__global__ __launch_bounds__(256) void k_km_accum(const float* __restrict__ x, long n, int d, int k, const int* __restrict__ assign,
                                                  const int* __restrict__ state, int DT, int Q, long chunk,
                                                  double* __restrict__ psum, long long* __restrict__ pcnt) {
    extern __shared__ __attribute__((aligned(16))) double km_acc[];
    if (state[0]) return;
    int* cnt = (int*)(km_acc + (size_t)Q * k * DT);
    const int nt = blockDim.x;
    for (int i = threadIdx.x; i < Q * k * DT; i += nt) km_acc[i] = 0.0;
    for (int i = threadIdx.x; i < Q * k; i += nt) cnt[i] = 0;
    __syncthreads();
    const int q = threadIdx.x / DT, jj = threadIdx.x - q * DT, j = (int)blockIdx.y * DT + jj;
    const long t_begin = (long)blockIdx.x * chunk;
    const long t_end = t_begin + chunk < n ? t_begin + chunk : n;
    if (q < Q && j < d) {
        const long sub = (chunk + Q - 1) / Q;
        const long t0 = t_begin + q * sub;
        const long t1 = t0 + sub < t_end ? t0 + sub : t_end;
        double* mine = km_acc + (size_t)q * k * DT + jj;
        const bool counter = blockIdx.y == 0 && jj == 0;
        for (long t = t0; t < t1; t += kKmAB) {
            int a[kKmAB];
            float v[kKmAB];
#pragma unroll
            for (int e = 0; e < kKmAB; ++e) {
                const bool in = t + e < t1;
                a[e] = in ? assign[t + e] : -1;
                v[e] = in ? x[(t + e) * d + j] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < kKmAB; ++e)
                if ((unsigned)a[e] < (unsigned)k) {
                    mine[a[e] * DT] += (double)v[e];
                    if (counter) ++cnt[q * k + a[e]];
                }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k * DT; i += nt) {
        const int c = i / DT, e = i - c * DT, col = (int)blockIdx.y * DT + e;
        if (col < d) {
            double sum = 0.0;
            for (int qq = 0; qq < Q; ++qq) sum += km_acc[((size_t)qq * k + c) * DT + e];
            psum[((size_t)blockIdx.x * k + c) * d + col] = sum;
        }
    }
    if (blockIdx.y == 0)
        for (int c = threadIdx.x; c < k; c += nt) {
            long long m = 0;
            for (int qq = 0; qq < Q; ++qq) m += cnt[qq * k + c];
            pcnt[(size_t)blockIdx.x * k + c] = m;
        }
}

// Workgroup: kKmFinE consecutive elements (c, j) of the k x d sums; thread (q, e) adds the splits q, q + kKmFinQ, ... in ascending
// order, the kKmFinQ sums meet in LDS and are added in the order of q (k_moments_finish's scheme).  Counts alike, in integers.
constexpr int kKmFinE = 16, kKmFinQ = 16;

__global__ __launch_bounds__(256) void k_km_finish(const double* __restrict__ psum, const long long* __restrict__ pcnt, int d, int k,
                                                   int S, const int* __restrict__ state, double* __restrict__ sums,
                                                   long long* __restrict__ counts, float* __restrict__ centers) {
    __shared__ double red[kKmFinQ][kKmFinE];
    __shared__ long long redc[kKmFinQ][kKmFinE];
    if (state[0]) return;
    const int el = threadIdx.x & (kKmFinE - 1), q = threadIdx.x / kKmFinE;
    const int e = blockIdx.x * kKmFinE + el;
    const bool in = e < k * d;
    const int c = in ? e / d : 0;
    double sum = 0.0;
    long long m = 0;
    if (in) {
#pragma unroll 4
        for (int sp = q; sp < S; sp += kKmFinQ) {
            sum += psum[(size_t)sp * k * d + e];
            m += pcnt[(size_t)sp * k + c];
        }
    }
    red[q][el] = sum;
    redc[q][el] = m;
    __syncthreads();
    if (q == 0 && in) {
        sum = red[0][el];
        m = redc[0][el];
        for (int qq = 1; qq < kKmFinQ; ++qq) {
            sum += red[qq][el];
            m += redc[qq][el];
        }
        sums[e] = sum;
        if (e == c * d) counts[c] = m;
        if (m > 0) centers[e] = (float)(sum / (double)m);
    }
}

__global__ __launch_bounds__(256) void k_km_update(const double* __restrict__ cost_partial, int groups, double tol,
                                                   double* __restrict__ cost, int* __restrict__ state) {
    __shared__ double red[256];
    if (state[0]) return;
    double v = 0.0;
    for (int i = threadIdx.x; i < groups; i += 256) v += cost_partial[i];
    const double now = km_block_sum(v, red);   // (every thread has read state[0] by here)
    if (threadIdx.x == 0) {
        const double prev = cost[0];
        const int steps = state[1];
        cost[1] = prev;
        cost[0] = now;
        state[1] = steps + 1;
        if (steps >= 1 && fabs(prev - now) <= tol * now) state[0] = 1;
    }
}

void launch_kmeans_step(long n, int d, int k, const float* x, float* centers, int32_t* assign, double* sums, int64_t* counts,
                        double* cost, int32_t* state, double tol, void* ws, hipStream_t s) {
    const KmAccShape a = km_acc_shape(n, d, k);
    const int groups = km_groups(n), kt = km_center_tile(d, k);
    double* cost_partial = (double*)ws;
    double* psum = cost_partial + kKmMaxGroups;
    long long* pcnt = (long long*)(psum + (size_t)a.S * k * d);
    hipLaunchKernelGGL(k_km_assign, dim3((unsigned)groups), dim3(256), (size_t)kt * km_row(d) * sizeof(float), s, x, n, d, k, kt,
                       (const float*)centers, (const int*)state, assign, (float*)nullptr, cost_partial);
    const size_t lds = (size_t)a.Q * k * a.DT * sizeof(double) + (size_t)a.Q * k * sizeof(int);
    hipLaunchKernelGGL(k_km_accum, dim3((unsigned)a.S, (unsigned)a.tiles), dim3((unsigned)((a.Q * a.DT + 63) & ~63)), lds, s, x, n, d, k, (const int*)assign,
                       (const int*)state, a.DT, a.Q, a.chunk, psum, pcnt);
    hipLaunchKernelGGL(k_km_finish, dim3((unsigned)((k * d + kKmFinE - 1) / kKmFinE)), dim3(256), 0, s, (const double*)psum,
                       (const long long*)pcnt, d, k, a.S, (const int*)state, sums, (long long*)counts, centers);
    hipLaunchKernelGGL(k_km_update, dim3(1), dim3(256), 0, s, (const double*)cost_partial, groups, tol, cost, state);
}

// ---- k-means++ ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pp_init(long n, long first, long long* __restrict__ chosen, float* __restrict__ mind2) {
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long)gridDim.x * 256) mind2[t] = __builtin_inff();
    if (blockIdx.x == 0 && threadIdx.x == 0) chosen[0] = first;
}

// mind2[t] = min(mind2[t], |x_t - x_chosen[r - 1]|^2), and seg[g] = the fp64 sum of segment g's 256 values in a fixed tree.
// Dynamic LDS: d floats, the chosen row.
__global__ __launch_bounds__(256) void k_pp_update(const float* __restrict__ x, long n, int d, const long long* __restrict__ chosen,
                                                   int r, float* __restrict__ mind2, double* __restrict__ seg) {
    extern __shared__ float pp_row[];
    __shared__ double red[256];
    long c = chosen[r - 1];
    c = c < 0 ? 0 : (c > n - 1 ? n - 1 : c);   // (a caller's index from outside stays inside x)
    for (int j = threadIdx.x; j < d; j += 256) pp_row[j] = x[c * d + j];
    __syncthreads();
    const long G = (n + kPpSeg - 1) / kPpSeg;
    for (long g = blockIdx.x; g < G; g += gridDim.x) {
        const long t = g * kPpSeg + threadIdx.x;
        double v = 0.0;
        if (t < n) {
            const float* xr = x + t * d;
            float acc = 0.f;
            for (int j = 0; j < d; ++j) {
                const float diff = xr[j] - pp_row[j];
                acc = fmaf(diff, diff, acc);
            }
            const float m = fminf(mind2[t], acc);
            mind2[t] = m;
            v = (double)m;
        }
        const double s = km_block_sum(v, red);
        if (threadIdx.x == 0) seg[g] = s;
    }
}

// One workgroup.  Thread i adds the segments of run i in order; thread 0 adds the runs in order (the total), then walks runs,
// the run's segments and the segment's points for the smallest index whose cumulative sum exceeds u * total.
__global__ __launch_bounds__(256) void k_pp_select(const float* __restrict__ mind2, const double* __restrict__ seg, long n, double u,
                                                   int r, long long* __restrict__ chosen) {
    __shared__ double runs[256];
    const long G = (n + kPpSeg - 1) / kPpSeg, RL = (G + 255) / 256;
    const long g0 = threadIdx.x * RL, g1 = g0 + RL < G ? g0 + RL : G;
    double v = 0.0;
    for (long g = g0; g < g1; ++g) v += seg[g];
    runs[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int i = 0; i < 256; ++i) total += runs[i];
    long pick = (long)floor(u * (double)n);
    pick = pick > n - 1 ? n - 1 : pick;
    if (total > 0.0) {
        const double target = u * total;
        double cum = 0.0;
        int run = 255;
        for (int i = 0; i < 256; ++i) {
            if (cum + runs[i] > target) {
                run = i;
                break;
            }
            cum += runs[i];
        }
        long sg0 = run * RL, sg1 = sg0 + RL < G ? sg0 + RL : G;
        if (sg0 >= G) sg0 = G - 1;   // (only when no run exceeded the target: a NaN among the values)
        long sgm = sg1 - 1 > sg0 ? sg1 - 1 : sg0;
        for (long g = sg0; g < sg1; ++g) {
            if (cum + seg[g] > target) {
                sgm = g;
                break;
            }
            cum += seg[g];
        }
        // the segment's own sum is a tree, this walk is sequential: where rounding lets the walk end below the target, the
        // segment's last point of non-zero weight is taken
        const long p0 = sgm * kPpSeg, p1 = p0 + kPpSeg < n ? p0 + kPpSeg : n;
        pick = p1 - 1;
        long last_pos = -1;
        for (long t = p0; t < p1; ++t) {
            const double w = (double)mind2[t];
            if (w > 0.0) last_pos = t;
            if (cum + w > target) {
                last_pos = t;
                break;
            }
            cum += w;
        }
        if (last_pos >= 0) pick = last_pos;
    }
    chosen[r] = pick;
}

void launch_kmeans_pp(long n, int d, const float* x, const double* u_host, int r0, int r1, int64_t* chosen, float* mind2, void* ws,
                      hipStream_t s) {
    const long G = (n + kPpSeg - 1) / kPpSeg;
    const unsigned grid = (unsigned)(G < (1l << 20) ? G : (1l << 20));
    double* seg = (double*)ws;
    for (int r = r0; r < r1; ++r) {
        if (r == 0) {
            long first = (long)std::floor(u_host[0] * (double)n);
            first = first > n - 1 ? n - 1 : first;
            hipLaunchKernelGGL(k_pp_init, dim3(grid), dim3(256), 0, s, n, first, (long long*)chosen, mind2);
            continue;
        }
        hipLaunchKernelGGL(k_pp_update, dim3(grid), dim3(256), (size_t)d * sizeof(float), s, x, n, d, (const long long*)chosen, r,
                           mind2, seg);
        hipLaunchKernelGGL(k_pp_select, dim3(1), dim3(256), 0, s, (const float*)mind2, (const double*)seg, n, u_host[r], r,
                           (long long*)chosen);
    }
}

// ---- count matrix ---------------------------------------------------------------------------------------------------
constexpr int kCmLdsCells = 12288;   // ints of LDS a private count matrix may take (48 KB): k <= 110

// blockIdx.x: pairs (t, t + lag), t in [x * chunk, (x + 1) * chunk), of the m = n - lag pairs.  Dynamic LDS: k * k ints, or none.
__global__ __launch_bounds__(256) void k_count_matrix(const int* __restrict__ dtraj, long m, long lag, int k, long chunk, int in_lds,
                                                      unsigned long long* __restrict__ counts, unsigned long long* __restrict__ dropped) {
    extern __shared__ int cm_cnt[];
    const int cells = k * k;
    if (in_lds) {
        for (int i = threadIdx.x; i < cells; i += 256) cm_cnt[i] = 0;
        __syncthreads();
    }
    const long t0 = (long)blockIdx.x * chunk;
    const long t1 = t0 + chunk < m ? t0 + chunk : m;
    int drop = 0;
    for (long t = t0 + threadIdx.x; t < t1; t += 256) {
        const int i = dtraj[t], j = dtraj[t + lag];
        if ((unsigned)i >= (unsigned)k || (unsigned)j >= (unsigned)k)
            ++drop;
        else if (in_lds)
            atomicAdd(&cm_cnt[i * k + j], 1);
        else
            atomicAdd(&counts[i * k + j], 1ull);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) drop += __shfl_xor(drop, o);
    if (in_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += 256)
            if (cm_cnt[i]) atomicAdd(&counts[i], (unsigned long long)cm_cnt[i]);
    }
    if ((threadIdx.x & 63) == 0 && drop) atomicAdd(dropped, (unsigned long long)drop);
}

// counts [k][k] and dropped [1] must be zero on entry; lag < n
void launch_count_matrix(long n, long lag, int k, const int32_t* dtraj, int64_t* counts, int64_t* dropped, hipStream_t s) {
    const long m = n - lag;
    const int in_lds = k * k <= kCmLdsCells;
    long chunk = in_lds ? 16384 : 4096;   // (a chunk's counts fit an int)
    if ((m + chunk - 1) / chunk > (1l << 20)) chunk = (m + (1l << 20) - 1) >> 20;
    hipLaunchKernelGGL(k_count_matrix, dim3((unsigned)((m + chunk - 1) / chunk)), dim3(256), in_lds ? (size_t)k * k * sizeof(int) : 0, s,
                       dtraj, m, lag, k, chunk, in_lds, (unsigned long long*)counts, (unsigned long long*)dropped);
}

}  // namespace mdg
