// k_ensemble.hip -- Cartesian ensemble statistics of protein trajectories (mdgen_ens_superpose / _moments / _pairwise_d2 /
// _contact_counts / _sasa_counts; mdgen_amd/ensemble.py): everything that scales with frames x atoms or frames x frames.  The 3 x 3 matrix
// square roots of the Gaussian Wasserstein distance, the PCA eigenproblem and the assignment problem are the host's.
//   k_superpose<W>   W waves own a frame (W = 1: four frames a workgroup, A <= 256; W = 4: a workgroup a frame).  Three passes over
//                    the frame's atoms, all sums fp64: the weighted centroids, H about them, then the rotated atoms and the rmsd.
//                    Every lane holds the same H and runs Horn's 4 x 4 Jacobi itself (ensemble.h): no broadcast, no divergence.
//                    A thread reads an atom before it writes it and touches no other thread's atoms after pass 2: out may be x
//   k_moments        workgroup (64 atoms, split of the frames): a thread owns (atom, quarter of the split) and adds
//                    u = x_t - x_0 and the six products u_i u_j in fp64, t ascending; the quarters, then k_moments_finish the
//                    splits, are added in order
//   k_pairwise_d2    GEMM-shaped: a workgroup walks tiles of 128 xa frames x 64 xb frames; 24 coordinates of each pass through LDS
//                    coordinate-major ([k][frame], rows padded by 4 floats), a thread owns 8 x 4 pairs and reads its 8 + 4 values
//                    of a coordinate as three ds_read_b128 (the xb ones conflict-free, 256 contiguous bytes a 16-lane group; the
//                    xa ones four addresses a wave, broadcast) for 32 subtractions and 32 FMAs.  Each pair is one FMA chain over
//                    the coordinates ascending, whatever the tiling.  sqrt(d2 / A) and d2 / A are added in fp64 per thread in pair
//                    order, per workgroup in a tree, and by k_pairwise_finish in workgroup order
//   k_contacts       workgroup (64 x 64 block of residue pairs on or above the diagonal, split of the frames): 8 frames of the
//                    two residue blocks pass through LDS axis-major, a thread counts its 4 x 4 pairs in registers and adds them
//                    to counts[i][j] (and counts[j][i] off the diagonal blocks) with integer atomics: exact in any order
//   k_sasa           Shrake-Rupley counts (mdgen_ens_sasa_counts): a wave owns an (frame, atom).  Its lanes scan the frame's atoms 64
//                    at a time and compact those within reach -- |c_i - c_j| < R_i + R_j, with slack -- by ballot into the wave's
//                    LDS list of (x, y, z, R2), 512 entries; then a lane owns every 64th sphere point, tests the neighbour that
//                    buried its previous point first and leaves the list at the first burying one.  A list that would overflow
//                    is dropped whole and every point is tested against all atoms.  Integers: exact in any order
// No floating-point atomics: every fp sum has a fixed order, two calls give the same bits.
#include "ensemble.h"
#include "kernels.h"

namespace mdg {

// ---- sums over the W waves that own a frame --------------------------------------------------------------------------
// Butterfly over the wave (a + b is commutative: every lane ends with the same bits), then the W wave sums in wave order.
template <int W, int NV>
__device__ __forceinline__ void ens_group_sum(double (&v)[NV], double* red) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o);
    if constexpr (W > 1) {
        const int wave = threadIdx.x >> 6;
        __syncthreads();   // (the previous sum's readers are done)
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            double s = red[i];
#pragma unroll
            for (int w = 1; w < W; ++w) s += red[w * NV + i];
            v[i] = s;
        }
    }
}

// ---- superposition ---------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_superpose(long F, int A, const float* x, const float* __restrict__ ref,
                                                   const float* __restrict__ w, const unsigned char* __restrict__ exists, float* out,
                                                   double* __restrict__ rot, double* __restrict__ rmsd) {
    __shared__ double red[W * 9];
    constexpr int G = 64 * W;                       // threads of a frame
    constexpr int FPB = 256 / G;                    // frames of a workgroup
    const int lane = threadIdx.x % G, sub = threadIdx.x / G;
    // (x and out carry no __restrict__: they may be one array)
    for (long f0 = (long)blockIdx.x * FPB; f0 < F; f0 += (long)gridDim.x * FPB) {
        const long f = f0 + sub;
        if (W == 1 && f >= F) continue;             // a wave of its own: no barrier is skipped (W = 4 has sub = 0 always)
        const float* xf = x + f * A * 3;
        double s7[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int a = lane; a < A; a += G) {
            const double wa = (double)w[a];
            s7[0] += wa;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                s7[1 + i] += wa * (double)xf[a * 3 + i];
                s7[4 + i] += wa * (double)ref[a * 3 + i];
            }
        }
        ens_group_sum<W, 7>(s7, red);
        double cx[3], cr[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cx[i] = s7[1 + i] / s7[0];
            cr[i] = s7[4 + i] / s7[0];
        }
        double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int a = lane; a < A; a += G) {
            const double wa = (double)w[a];
            double p[3], q[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                p[i] = (double)xf[a * 3 + i] - cx[i];
                q[i] = (double)ref[a * 3 + i] - cr[i];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) H[3 * i + j] += wa * (p[i] * q[j]);   // (x == ref: H symmetric to the bit)
        }
        ens_group_sum<W, 9>(H, red);
        double R[9];
        horn_rotation(H, R);
        float Rf[9], cxf[3], crf[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rf[i] = (float)R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cxf[i] = (float)cx[i];
            crf[i] = (float)cr[i];
        }
        double dev[1] = {0.0};
        float* of = out + f * A * 3;
        for (int a = lane; a < A; a += G) {
            const float xv[3] = {xf[a * 3], xf[a * 3 + 1], xf[a * 3 + 2]};
            const double wa = (double)w[a];
            if (rmsd && wa != 0.0) {
                const double p[3] = {(double)xv[0] - cx[0], (double)xv[1] - cx[1], (double)xv[2] - cx[2]};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double e = R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] - ((double)ref[a * 3 + i] - cr[i]);
                    dev[0] += wa * e * e;
                }
            }
            if (!exists || exists[a]) {
                const float d0 = xv[0] - cxf[0], d1 = xv[1] - cxf[1], d2 = xv[2] - cxf[2];
#pragma unroll
                for (int i = 0; i < 3; ++i) of[a * 3 + i] = fmaf(Rf[3 * i], d0, fmaf(Rf[3 * i + 1], d1, fmaf(Rf[3 * i + 2], d2, crf[i])));
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) of[a * 3 + i] = xv[i];
            }
        }
        if (rmsd) {
            ens_group_sum<W, 1>(dev, red);
            if (lane == 0) rmsd[f] = sqrt(dev[0] / s7[0]);
        }
        if (rot && lane == 0)
#pragma unroll
            for (int i = 0; i < 9; ++i) rot[f * 9 + i] = R[i];
    }
}

void launch_ens_superpose(long F, int A, const float* x, const float* ref, const float* w, const uint8_t* exists, float* out,
                          double* rot, double* rmsd, hipStream_t s) {
    if (A <= kEnsWaveAtoms) {
        const long g = (F + 3) / 4;
        hipLaunchKernelGGL(k_superpose<1>, dim3((unsigned)(g < (1l << 20) ? g : (1l << 20))), dim3(256), 0, s, F, A, x, ref, w, exists,
                           out, rot, rmsd);
    } else {
        hipLaunchKernelGGL(k_superpose<4>, dim3((unsigned)(F < (1l << 20) ? F : (1l << 20))), dim3(256), 0, s, F, A, x, ref, w, exists,
                           out, rot, rmsd);
    }
}

// ---- per-atom mean and covariance ------------------------------------------------------------------------------------
constexpr int kMoAtoms = 64;               // atoms of a workgroup; x 4 quarters of its frame split
constexpr long kMoMaxPartialAtoms = 1l << 18;   // splits x A at the most: 18 MB of partials
constexpr int kMoMaxSplits = 256;

int ens_moments_splits(long F, int A) {
    long S = kMoMaxPartialAtoms / A;
    S = S > kMoMaxSplits ? kMoMaxSplits : S;
    const long runs = (F + 255) / 256;       // no split shorter than 256 frames (64 a quarter)
    S = S > runs ? runs : S;
    S = S < 1 ? 1 : S;
    const long chunk = (F + S - 1) / S;
    return (int)((F + chunk - 1) / chunk);   // no empty split
}

// partial [S][A][9] fp64: sum u (3), then sum of u0 u0, u0 u1, u0 u2, u1 u1, u1 u2, u2 u2
size_t ens_moments_workspace_bytes(long F, int A) { return (size_t)ens_moments_splits(F, A) * A * 9 * sizeof(double); }

__global__ __launch_bounds__(256) void k_moments(long F, int A, const float* __restrict__ x, long chunk, double* __restrict__ partial) {
    __shared__ double red[3][kMoAtoms][9];
    const int al = threadIdx.x % kMoAtoms, qu = threadIdx.x / kMoAtoms;
    const int a = blockIdx.x * kMoAtoms + al;
    const long t0 = (long)blockIdx.y * chunk, t1 = t0 + chunk < F ? t0 + chunk : F;
    const long quarter = (t1 - t0 + 3) / 4;
    const long q0 = t0 + qu * quarter, q1 = q0 + quarter < t1 ? q0 + quarter : t1;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (a < A) {
        const double o0 = (double)x[a * 3], o1 = (double)x[a * 3 + 1], o2 = (double)x[a * 3 + 2];
        for (long t = q0; t < q1; ++t) {
            const float* p = x + (t * A + a) * 3;
            const double u0 = (double)p[0] - o0, u1 = (double)p[1] - o1, u2 = (double)p[2] - o2;
            acc[0] += u0;
            acc[1] += u1;
            acc[2] += u2;
            acc[3] += u0 * u0;
            acc[4] += u0 * u1;
            acc[5] += u0 * u2;
            acc[6] += u1 * u1;
            acc[7] += u1 * u2;
            acc[8] += u2 * u2;
        }
    }
    if (qu > 0)
#pragma unroll
        for (int i = 0; i < 9; ++i) red[qu - 1][al][i] = acc[i];
    __syncthreads();
    if (qu == 0 && a < A)
#pragma unroll
        for (int i = 0; i < 9; ++i) partial[((long)blockIdx.y * A + a) * 9 + i] = ((acc[i] + red[0][al][i]) + red[1][al][i]) + red[2][al][i];
}

__global__ __launch_bounds__(256) void k_moments_finish(long F, int A, int S, const float* __restrict__ x,
                                                        const double* __restrict__ partial, double* __restrict__ mean,
                                                        double* __restrict__ cov) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    double s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = partial[(long)a * 9 + i];
    for (int sp = 1; sp < S; ++sp)
#pragma unroll
        for (int i = 0; i < 9; ++i) s[i] += partial[((long)sp * A + a) * 9 + i];
    const double n = (double)F;
    const double m[3] = {s[0] / n, s[1] / n, s[2] / n};
#pragma unroll
    for (int i = 0; i < 3; ++i) mean[a * 3 + i] = (double)x[a * 3 + i] + m[i];
    const double c00 = s[3] / n - m[0] * m[0], c01 = s[4] / n - m[0] * m[1], c02 = s[5] / n - m[0] * m[2];
    const double c11 = s[6] / n - m[1] * m[1], c12 = s[7] / n - m[1] * m[2], c22 = s[8] / n - m[2] * m[2];
    double* c = cov + (long)a * 9;
    c[0] = c00;
    c[1] = c01;
    c[2] = c02;
    c[3] = c01;
    c[4] = c11;
    c[5] = c12;
    c[6] = c02;
    c[7] = c12;
    c[8] = c22;
}

void launch_ens_moments(long F, int A, const float* x, double* mean, double* cov, void* ws, hipStream_t s) {
    const int S = ens_moments_splits(F, A);
    const long chunk = (F + S - 1) / S;
    double* partial = (double*)ws;
    hipLaunchKernelGGL(k_moments, dim3((A + kMoAtoms - 1) / kMoAtoms, S), dim3(256), 0, s, F, A, x, chunk, partial);
    hipLaunchKernelGGL(k_moments_finish, dim3((A + 255) / 256), dim3(256), 0, s, F, A, S, x, (const double*)partial, mean, cov);
}

// ---- all-pairs squared distances -------------------------------------------------------------------------------------
constexpr int kPdRowA = kEnsPairTileA + 4, kPdRowB = kEnsPairTileB + 4;   // LDS rows: + 16 bytes, so that the transposing writes of
                                                                           // one frame's 24 coordinates spread over 8 banks, not 1
constexpr int kPdMaxGroups = 65536;

static long pd_tiles(long Fa, long Fb) {
    return ((Fa + kEnsPairTileA - 1) / kEnsPairTileA) * ((Fb + kEnsPairTileB - 1) / kEnsPairTileB);
}
static int pd_groups(long Fa, long Fb) {
    const long t = pd_tiles(Fa, Fb);
    return (int)(t < kPdMaxGroups ? t : kPdMaxGroups);
}

// partial [groups][2] fp64
size_t ens_pairwise_workspace_bytes(long Fa, long Fb) { return (size_t)pd_groups(Fa, Fb) * 2 * sizeof(double); }

// n rows of `x` from row r0 on, coordinates k0 .. k0 + kEnsPairChunk of the D of a row, into dst[k][row] (zero beyond either end)
template <int ROWS, int STRIDE>
__device__ __forceinline__ void pd_stage(const float* __restrict__ x, long F, int D, long r0, int k0, float* dst) {
    for (int e = threadIdx.x; e < ROWS * kEnsPairChunk; e += 256) {
        const int r = e / kEnsPairChunk, k = e % kEnsPairChunk;
        const long row = r0 + r;
        dst[k * STRIDE + r] = (row < F && k0 + k < D) ? x[row * D + k0 + k] : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_pairwise_d2(long Fa, long Fb, int A, const float* __restrict__ xa, const float* __restrict__ xb,
                                                     float* __restrict__ d2, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float sa[kEnsPairChunk * kPdRowA], sb[kEnsPairChunk * kPdRowB];
    __shared__ double red[2][256];
    const int D = 3 * A;
    const long tiles_b = (Fb + kEnsPairTileB - 1) / kEnsPairTileB;
    const long tiles = ((Fa + kEnsPairTileA - 1) / kEnsPairTileA) * tiles_b;
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;   // pairs (8 ty + i, 4 tx + j) of the tile
    const double inv_a = 1.0 / (double)A;
    double s_root = 0.0, s_sq = 0.0;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long a0 = (tile / tiles_b) * kEnsPairTileA, b0 = (tile % tiles_b) * kEnsPairTileB;
        float acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        for (int k0 = 0; k0 < D; k0 += kEnsPairChunk) {
            __syncthreads();
            pd_stage<kEnsPairTileA, kPdRowA>(xa, Fa, D, a0, k0, sa);
            pd_stage<kEnsPairTileB, kPdRowB>(xb, Fb, D, b0, k0, sb);
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < kEnsPairChunk; ++k) {
                const float4 p0 = *(const float4*)&sa[k * kPdRowA + 8 * ty], p1 = *(const float4*)&sa[k * kPdRowA + 8 * ty + 4];
                const float4 q = *(const float4*)&sb[k * kPdRowB + 4 * tx];
                const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
                const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float diff = pv[i] - qv[j];
                        acc[i][j] = fmaf(diff, diff, acc[i][j]);
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long ra = a0 + 8 * ty + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long rb = b0 + 4 * tx + j;
                if (ra < Fa && rb < Fb) {
                    const double m = (double)acc[i][j] * inv_a;
                    s_root += sqrt(m);
                    s_sq += m;
                    if (d2) d2[ra * Fb + rb] = acc[i][j];
                }
            }
        }
    }
    red[0][threadIdx.x] = s_root;
    red[1][threadIdx.x] = s_sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = red[0][0];
        partial[2 * blockIdx.x + 1] = red[1][0];
    }
}

__global__ __launch_bounds__(256) void k_pairwise_finish(int groups, const double* __restrict__ partial, double* __restrict__ sums) {
    __shared__ double red[2][256];
    double s0 = 0.0, s1 = 0.0;
    for (int g = threadIdx.x; g < groups; g += 256) {
        s0 += partial[2 * g];
        s1 += partial[2 * g + 1];
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[0] = red[0][0];
        sums[1] = red[1][0];
    }
}

void launch_ens_pairwise_d2(long Fa, long Fb, int A, const float* xa, const float* xb, float* d2, double* sums, void* ws,
                            hipStream_t s) {
    const int groups = pd_groups(Fa, Fb);
    double* partial = (double*)ws;
    hipLaunchKernelGGL(k_pairwise_d2, dim3(groups), dim3(256), 0, s, Fa, Fb, A, xa, xb, d2, partial);
    hipLaunchKernelGGL(k_pairwise_finish, dim3(1), dim3(256), 0, s, groups, (const double*)partial, sums);
}

// ---- contact counts --------------------------------------------------------------------------------------------------
constexpr int kCcTile = 64;      // residues of a block
constexpr int kCcFrames = 8;     // frames staged at a time
constexpr int kCcTargetGroups = 4096;

// residues i0 .. i0 + 63 of frames t0 .. t0 + 7 into dst[frame][axis][residue]; beyond N or t1: zeros (their counts are dropped)
__device__ __forceinline__ void cc_stage(const float* __restrict__ ca, int N, long t0, long t1, int i0, float* dst) {
    for (int e = threadIdx.x; e < kCcFrames * kCcTile * 3; e += 256) {
        const int fr = e / (kCcTile * 3), r = e % (kCcTile * 3);
        const int res = r / 3, ax = r % 3;
        const long t = t0 + fr;
        dst[(fr * 3 + ax) * kCcTile + res] = (t < t1 && i0 + res < N) ? ca[(t * N + i0 + res) * 3 + ax] : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_contacts(long F, int N, const float* __restrict__ ca, float cutoff2, long chunk, int nb,
                                                  int* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float si[kCcFrames * 3 * kCcTile], sj[kCcFrames * 3 * kCcTile];
    // blockIdx.x: the block pair (bi <= bj), row by row of the upper triangle
    int bi = 0, rest = blockIdx.x;
    while (rest >= nb - bi) {
        rest -= nb - bi;
        ++bi;
    }
    const int bj = bi + rest;
    const int i0 = bi * kCcTile, j0 = bj * kCcTile;
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    const long t_begin = (long)blockIdx.y * chunk, t_end = t_begin + chunk < F ? t_begin + chunk : F;
    int cnt[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt[i][j] = 0;
    for (long t0 = t_begin; t0 < t_end; t0 += kCcFrames) {
        __syncthreads();
        cc_stage(ca, N, t0, t_end, i0, si);
        cc_stage(ca, N, t0, t_end, j0, sj);
        __syncthreads();
        const int nf = t_end - t0 < kCcFrames ? (int)(t_end - t0) : kCcFrames;
        // (vectorised across frames, the loop's fp32 math comes out as v_pk_*_f32, which the build refuses)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int fr = 0; fr < nf; ++fr) {
            float pi[3][4], pj[3][4];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float4 u = *(const float4*)&si[(fr * 3 + ax) * kCcTile + 4 * ty];
                const float4 v = *(const float4*)&sj[(fr * 3 + ax) * kCcTile + 4 * tx];
                pi[ax][0] = u.x, pi[ax][1] = u.y, pi[ax][2] = u.z, pi[ax][3] = u.w;
                pj[ax][0] = v.x, pj[ax][1] = v.y, pj[ax][2] = v.z, pj[ax][3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dx = pi[0][i] - pj[0][j], dy = pi[1][i] - pj[1][j], dz = pi[2][i] - pj[2][j];
                    const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    cnt[i][j] += dd < cutoff2 ? 1 : 0;
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = i0 + 4 * ty + i, gj = j0 + 4 * tx + j;
            if (gi < N && gj < N && cnt[i][j]) {
                atomicAdd(&counts[(long)gi * N + gj], cnt[i][j]);
                if (bi != bj) atomicAdd(&counts[(long)gj * N + gi], cnt[i][j]);   // (dx * dx and its mirror are the same bits)
            }
        }
}

// counts [N][N] must be zero on entry
void launch_ens_contact_counts(long F, int N, const float* ca, float cutoff2, int32_t* counts, hipStream_t s) {
    const int nb = (N + kCcTile - 1) / kCcTile;
    const int pairs = nb * (nb + 1) / 2;
    long S = kCcTargetGroups / pairs;
    const long runs = (F + 63) / 64;     // no split shorter than 64 frames
    S = S > runs ? runs : S;
    S = S < 1 ? 1 : S;
    const long chunk = (F + S - 1) / S;
    S = (F + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_contacts, dim3(pairs, (unsigned)S), dim3(256), 0, s, F, N, ca, cutoff2, chunk, nb, counts);
}

// ---- Shrake-Rupley solvent-accessible surface ------------------------------------------------------------------------
constexpr int kSasaWaves = 4;                // waves of a workgroup, an atom each
constexpr long kSasaMaxGroups = 1l << 20;
// The cull keeps j when |c_i - c_j| <= (R_i + R_j) kSasaCullScale + kSasaCullAbs (max |coordinate| + 32).  A point of i is within
// R_i (1 + 1e-3) (the unit tolerance of the points) + sqrt(3) 2^-24 max|q| (its rounding) of c_i, and a burying j within
// R_j (1 + a few 2^-24) of the point: every such j is closer to i than the cut, whose own fp32 rounding is a few 2^-24 relative.
constexpr float kSasaCullScale = 1.002f;
constexpr float kSasaCullAbs = 4e-7f;

// workspace, fp32: R [A] (0: no atom), R2 [A], then the points axis-major, px [P], py [P], pz [P]
size_t ens_sasa_workspace_bytes(int A, int P) { return (((size_t)2 * A + (size_t)3 * P) * sizeof(float) + 15) / 16 * 16; }

// writes made by the wave's lanes to its own LDS list are read by its other lanes from here on (LDS is in order within a wave)
__device__ __forceinline__ void sasa_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool sasa_buries(float qx, float qy, float qz, float4 nb) {
    const float dx = qx - nb.x, dy = qy - nb.y, dz = qz - nb.z;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx)) < nb.w;
}

__global__ __launch_bounds__(256) void k_sasa(long F, int A, int P, const float* __restrict__ x, const float* __restrict__ R,
                                              const float* __restrict__ R2, const float* __restrict__ px,
                                              const float* __restrict__ py, const float* __restrict__ pz, int* __restrict__ counts) {
    __shared__ float4 lists[kSasaWaves][kEnsSasaMaxNeighbours];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4* list = lists[wave];
    const long total = F * (long)A;
    // (no workgroup barrier below: the waves' trip counts differ)
    for (long item = (long)blockIdx.x * kSasaWaves + wave; item < total; item += (long)gridDim.x * kSasaWaves) {
        const long f = item / A;
        const int i = (int)(item - f * A);
        const float Ri = R[i];
        if (Ri == 0.f) {                     // no atom here (the same for every lane)
            if (lane == 0) counts[item] = 0;
            continue;
        }
        const float* xf = x + f * A * 3;
        const float cx = xf[3 * i], cy = xf[3 * i + 1], cz = xf[3 * i + 2];
        const float mi = fmaxf(fmaxf(fabsf(cx), fabsf(cy)), fabsf(cz));
        // the atoms that can bury a point of i, compacted by ballot in atom order; more than the list holds: none is kept and
        // every point is tested against all atoms instead
        int cnt = 0;
        bool over = false;
        for (int j0 = 0; j0 < A; j0 += 64) {
            const int j = j0 + lane;
            bool keep = false;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (j < A) {
                const float Rj = R[j];
                v.x = xf[3 * j], v.y = xf[3 * j + 1], v.z = xf[3 * j + 2], v.w = R2[j];
                const float dx = cx - v.x, dy = cy - v.y, dz = cz - v.z;
                const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                const float m = fmaxf(mi, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fabsf(v.z)));
                const float cut = fmaf(Ri + Rj, kSasaCullScale, kSasaCullAbs * (m + 32.f));
                keep = Rj != 0.f && j != i && !(dd > cut * cut);   // (a NaN distance is kept: it buries nothing either way)
            }
            const unsigned long long mask = __ballot(keep);
            const int n = __popcll(mask);
            if (cnt + n > kEnsSasaMaxNeighbours) {
                over = true;
                break;
            }
            if (keep) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = v;
            cnt += n;
        }
        sasa_wave_sync();
        int open = 0, last = 0;
        for (int k0 = 0; k0 < P; k0 += 64) {
            const int k = k0 + lane;
            bool exposed = false;
            if (k < P) {
                const float qx = fmaf(Ri, px[k], cx), qy = fmaf(Ri, py[k], cy), qz = fmaf(Ri, pz[k], cz);
                bool buried = false;
                if (!over) {
                    if (cnt > 0) buried = sasa_buries(qx, qy, qz, list[last]);   // what buried this lane's previous point
                    for (int n = 0; n < cnt && !buried; ++n)
                        if (sasa_buries(qx, qy, qz, list[n])) {
                            buried = true;
                            last = n;
                        }
                } else {
                    for (int j = 0; j < A && !buried; ++j) {    // (R2 = 0 where no atom is: d2 < 0 never holds)
                        const float4 v = {xf[3 * j], xf[3 * j + 1], xf[3 * j + 2], R2[j]};
                        buried = j != i && sasa_buries(qx, qy, qz, v);
                    }
                }
                exposed = !buried;
            }
            open += __popcll(__ballot(exposed));
        }
        if (lane == 0) counts[item] = open;
        sasa_wave_sync();                    // the list is read to the end before the next atom's is written
    }
}

void launch_ens_sasa_counts(long F, int A, int P, const float* x, const float* ws, int32_t* counts, hipStream_t s) {
    const float *R = ws, *R2 = ws + A, *px = ws + 2 * (size_t)A, *py = px + P, *pz = py + P;
    const long g = (F * (long)A + kSasaWaves - 1) / kSasaWaves;
    hipLaunchKernelGGL(k_sasa, dim3((unsigned)(g < kSasaMaxGroups ? g : kSasaMaxGroups)), dim3(256), 0, s, F, A, P, x, R, R2, px, py,
                       pz, counts);
}

}  // namespace mdg
