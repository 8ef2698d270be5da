// analysis.h -- device code shared by k_analysis.hip and k_tica.hip: the histogram bin search and the direct autocovariance of one
// row (a plain series) or of two rows summed (the sin and the cos of an angle).
#pragma once
#include "kernels.h"

namespace mdg {

// searchsorted(e, x, 'right') - 1 with x == e[bins] in the last bin; -1: outside [e[0], e[bins]] (or NaN).  The guess is the
// uniform-bin arithmetic, the table decides.
__device__ __forceinline__ int hist_bin(double x, const double* __restrict__ e, int bins) {
    const double lo = e[0], hi = e[bins];
    if (!(x >= lo && x <= hi)) return -1;
    int b = hi > lo ? (int)((x - lo) / (hi - lo) * bins) : 0;
    b = b < 0 ? 0 : (b > bins - 1 ? bins - 1 : b);
    while (b > 0 && x < e[b]) --b;
    while (b < bins - 1 && x >= e[b + 1]) ++b;
    return b;
}

// ---- autocovariance -------------------------------------------------------------------------------------------------
constexpr int kAcTT = 2048;                     // samples t of a time tile
constexpr int kAcLB = 256;                      // lags of a lag block
constexpr int kAcR = 8;                         // lags per thread (and samples per inner step)
constexpr int kAcGroups = kAcLB / kAcR;         // 32 lag groups ...
constexpr int kAcStrips = 256 / kAcGroups;      // ... x 8 strips of the tile
constexpr int kAcStrip = kAcTT / kAcStrips;     // 256 samples: the length of an fp32 partial sum (x 2: sin and cos)
constexpr int kAcWin = kAcTT + kAcLB;           // floats of a tile's lag window ...
constexpr int kAcWinPad = kAcWin + 4 * (kAcWin / 64);   // ... and with 16 bytes of padding behind every 256 (ac_win)

// Where float i of the lag window lives.  A lane reads its 8 new window values as two ds_read_b128, lanes 32 bytes apart: unpadded,
// lanes l and l + 8 of a 16-lane group meet on one bank (256 bytes apart); the padding moves lane l + 8 to the other half of the slot.
__device__ __forceinline__ int ac_win(int i) { return i + 4 * (i >> 6); }

// acc[r] += sum_u a[u] * w[u + r]: 8 samples x 8 lags from 8 + 16 registers
__device__ __forceinline__ void ac_block(const float4& a0, const float4& a1, const float4& l0, const float4& l1, const float4& h0,
                                         const float4& h1, float (&acc)[kAcR]) {
    const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const float w[16] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w, h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int r = 0; r < kAcR; ++r) acc[r] = fmaf(a[u], w[u + r], acc[r]);
}

// Workgroup (lag block lb, split sp, feature f): lags k0 .. k0 + 255, time tiles sp, sp + S, ... of those that hold a t with
// t + k0 < n.  A tile stages x[t0 .. t0 + TT) and x[t0 + k0 .. t0 + k0 + TT + LB) of the row (ROWS 2: of the sin and of the cos row,
// whose products are summed), zero beyond n: the products past the series' end vanish without a branch.  Thread (strip st, lag group
// lg) walks 256 samples of the tile 8 at a time against a 16-wide sliding window, for its 8 lags.
// fp32 sums: ROWS 2 over the strip's 256 samples (x 2 rows) -- sin and cos products change sign and stay below 1.  ROWS 1 over 8
// samples only: a series with an offset has products of one sign, and adding near-equal terms one by one in fp32 rounds the same
// way every time (a constant 1.7: 3e-6 relative over 256 terms, 16 x what np.dot's blocked sum loses).
template <int ROWS>
__device__ __forceinline__ void acov_body(const float* S, const float* Cc, long n, long K, int splits, int lag_blocks,
                                          double* partial) {   // (__restrict__ is the kernels': here it would change their schedule)
    constexpr bool two = ROWS == 2;
    __shared__ __attribute__((aligned(16))) float aS[kAcTT], aC[two ? kAcTT : 4], bS[kAcWinPad], bC[two ? kAcWinPad : 4];
    __shared__ double red[kAcStrips][kAcLB];
    const long bid = blockIdx.x;
    const int lb = (int)(bid % lag_blocks);
    const int sp = (int)((bid / lag_blocks) % splits);
    const long f = bid / ((long)lag_blocks * splits);
    const long k0 = (long)lb * kAcLB;
    const long tiles = (n - k0 + kAcTT - 1) / kAcTT;   // k0 <= K <= n - 1: at least one
    const int lg = threadIdx.x & (kAcGroups - 1), st = threadIdx.x / kAcGroups;
    const float* rowS = S + f * n;
    const float* rowC = two ? Cc + f * n : nullptr;
    double acc64[kAcR];
#pragma unroll
    for (int r = 0; r < kAcR; ++r) acc64[r] = 0.0;
    for (long tile = sp; tile < tiles; tile += splits) {
        const long t0 = tile * kAcTT;
        __syncthreads();
        for (int i = threadIdx.x; i < kAcTT; i += 256) {
            const long g = t0 + i;
            aS[i] = g < n ? rowS[g] : 0.f;
            if constexpr (two) aC[i] = g < n ? rowC[g] : 0.f;
        }
        for (int i = threadIdx.x; i < kAcTT + kAcLB; i += 256) {
            const long g = t0 + k0 + i;
            bS[ac_win(i)] = g < n ? rowS[g] : 0.f;
            if constexpr (two) bC[ac_win(i)] = g < n ? rowC[g] : 0.f;
        }
        __syncthreads();
        float acc[kAcR];
#pragma unroll
        for (int r = 0; r < kAcR; ++r) acc[r] = 0.f;
        const float4* pa = (const float4*)(aS + st * kAcStrip);
        const float4* pc = (const float4*)(aC + (two ? st * kAcStrip : 0));
        const int w0 = st * kAcStrip + lg * kAcR;   // the thread's window starts here; last read: float 1792 + 248 + 248 + 15 = 2303
        float4 ls0 = *(const float4*)(bS + ac_win(w0)), ls1 = *(const float4*)(bS + ac_win(w0) + 4);
        float4 lc0 = ls0, lc1 = ls1;
        if constexpr (two) {
            lc0 = *(const float4*)(bC + ac_win(w0));
            lc1 = *(const float4*)(bC + ac_win(w0) + 4);
        }
#pragma unroll 2
        for (int j = 0; j < kAcStrip / 8; ++j) {
            const int w = ac_win(w0 + 8 * j + 8);    // (8 floats from a multiple of 8 never straddle a pad)
            const float4 hs0 = *(const float4*)(bS + w), hs1 = *(const float4*)(bS + w + 4);
            float4 hc0 = hs0, hc1 = hs1;
            if constexpr (two) {
                hc0 = *(const float4*)(bC + w);
                hc1 = *(const float4*)(bC + w + 4);
            }
            ac_block(pa[2 * j], pa[2 * j + 1], ls0, ls1, hs0, hs1, acc);
            if constexpr (two) ac_block(pc[2 * j], pc[2 * j + 1], lc0, lc1, hc0, hc1, acc);
            ls0 = hs0;
            ls1 = hs1;
            lc0 = hc0;
            lc1 = hc1;
            if constexpr (!two) {   // a plain series has an offset: see the head comment
#pragma unroll
                for (int r = 0; r < kAcR; ++r) {
                    acc64[r] += (double)acc[r];
                    acc[r] = 0.f;
                }
            }
        }
        if constexpr (two) {
#pragma unroll
            for (int r = 0; r < kAcR; ++r) acc64[r] += (double)acc[r];
        }
    }
#pragma unroll
    for (int r = 0; r < kAcR; ++r) red[st][lg * kAcR + r] = acc64[r];
    __syncthreads();
    const long k = k0 + threadIdx.x;
    if (k <= K) {
        double sum = red[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < kAcStrips; ++q) sum += red[q][threadIdx.x];
        partial[(f * splits + sp) * (K + 1) + k] = sum;   // every (f, sp, k) is written: zero where the split has no tile
    }
}

}  // namespace mdg
