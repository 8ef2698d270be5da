// k_rk.hip -- the device side of the fixed-grid Runge-Kutta sampler (ode.inc: midpoint, heun3, rk4 on t = linspace(0, 1, S + 1)).
//   k_rk_embed   the token embedding (k_embed, k_small.hip) of a state that exists only inside the launch: the staging prologue forms
//                the token's D values from y0 and up to four velocities (RkState), stages them in LDS and embeds them.  The first stage
//                of step i + 1 is the launch that forms y1 of step i: it also stores y1 over y0.
//   k_rk_update  the same arithmetic without the embedding: the result of the last step.
// A network evaluation outside the Euler graph otherwise starts with k_embed reading a state that a separate k_ode_combine launch
// has just written: one launch and one round trip of the state through HBM per evaluation.
// Every written operation of a state is one rounded fp32 operation (the formulas are torchdiffeq's fixed_grid.py / rk_common.py,
// restated in ode.inc): nothing is contracted into an FMA.
#include "kernels.h"

#pragma clang fp contract(off)

namespace mdg {

__device__ __forceinline__ float rk_state(const RkState& s, float y0, float k0, float k1, float k2, float k3) {
    switch (s.form) {
    case kRkAxk: return y0 + k0 * s.c[0];
    case kRkDtCk: return y0 + s.dt * (s.c[0] * k0);
    case kRkDtkC: return y0 + (s.dt * k0) * s.c[0];
    case kRkDtLin2: return y0 + s.dt * (s.c[0] * k0 + s.c[1] * k1);
    case kRkDtLin3: return y0 + s.dt * ((s.c[0] * k0 + s.c[1] * k1) + s.c[2] * k2);
    case kRk38: return y0 + (((k0 + s.c[0] * (k1 + k2)) + k3) * s.dt) * s.c[1];
    default: return y0;
    }
}

// k_embed's tile geometry (k_small.hip): 29-float LDS rows, 14 k-steps of v_mfma_f32_32x32x2_f32, the packed B operands of
// launch_pack_embed; workgroups of 128 tokens, or of 32 for the small launches.
constexpr int kEmbLd = 29, kEmbK = 14;
template <bool POS, bool IPA, int kEmbTok>
__global__ __launch_bounds__(256) void k_rk_embed(const EmbedParams p, const RkState st) {
    __shared__ float xs[kEmbTok * kEmbLd];
    __shared__ float cs[kEmbTok * kEmbLd];
    __shared__ int ms[kEmbTok];     // bit0: x_cond_mask, bit1: x_cond row has a non-zero
    __shared__ int tpos[kEmbTok];   // l * kC                 (row of pos_embed)
    __shared__ int tipa[kEmbTok];   // (b * L + l) * kC       (row of ipa_out)
    const int tid = threadIdx.x;
    const long tok0 = (long)blockIdx.x * kEmbTok;
    if (tid < kEmbTok) {
        long t = tok0 + tid;
        t = t < p.N ? t : p.N - 1;
        const int l = (int)(t % p.L), b = (int)(t / ((long)p.T * p.L));
        ms[tid] = 0;
        tpos[tid] = l * kC;
        tipa[tid] = (b * p.L + l) * kC;
    }
    __syncthreads();
    {   // stage the state / x_cond rows: unconditional clamped loads of y0, the velocities and x_cond, all in flight together
        constexpr int NIT = (kEmbTok * 28 + 255) / 256;
        float a[NIT], b[NIT], kv[kRkMaxK][NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i0 = tid + 256 * it;
            const int i = i0 < kEmbTok * 28 ? i0 : kEmbTok * 28 - 1;
            const int tk = i / 28, d = i % 28;
            long t = tok0 + tk;
            t = t < p.N ? t : p.N - 1;
            const int dc = d < p.D ? d : 0;
            const long e = t * p.D + dc;
            a[it] = st.y[e];
            b[it] = p.x_cond[e];
#pragma unroll
            for (int j = 0; j < kRkMaxK; ++j) kv[j][it] = j < st.nk ? st.k[j][e] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + 256 * it;
            if (i >= kEmbTok * 28) break;
            const int tk = i / 28, d = i % 28;
            const bool ok = tok0 + tk < p.N && d < p.D;
            const float v = rk_state(st, a[it], kv[0][it], kv[1][it], kv[2][it], kv[3][it]);
            xs[tk * kEmbLd + d] = ok ? v : 0.f;
            cs[tk * kEmbLd + d] = ok ? b[it] : 0.f;
            if (ok && b[it] != 0.f) atomicOr(&ms[tk], 2);
            // y1 over y0: element (token, d) is read and written by this thread alone (the clamped loads of other threads are discarded)
            if (st.store && ok) st.y[(tok0 + tk) * p.D + d] = v;
        }
    }
    const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id(), hh = lane >> 5, j = lane & 31;
    const int nk = (p.D + 1) >> 1;
    float wl[3][kEmbK], wc[3][kEmbK], b0[3], me0[3], me1[3];
#pragma unroll
    for (int ct = 0; ct < 3; ++ct) {
        const int c = 96 * w + 32 * ct + j;
#pragma unroll
        for (int ks = 0; ks < kEmbK; ++ks) {
            const int o = ((w * 3 + ct) * kEmbK + ks) * 64 + lane;
            wl[ct][ks] = p.wl_pack[o];
            wc[ct][ks] = p.wc_pack[o];
        }
        b0[ct] = p.bl[c] + p.bc[c];
        me0[ct] = p.mask_emb[c];
        me1[ct] = p.mask_emb[kC + c];
    }
    __syncthreads();
    if (tid < kEmbTok) {
        const long t = tok0 + tid;
        if (t < p.N && p.x_cond_mask[t]) ms[tid] |= 1;
    }
    __syncthreads();
#pragma unroll 1
    for (int rt = 0; rt < kEmbTok / 32; ++rt) {
        if (tok0 + rt * 32 >= p.N) break;
        f32x16 acc[3];
#pragma unroll
        for (int ct = 0; ct < 3; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
        const float* xr = xs + (rt * 32 + j) * kEmbLd + hh;
#pragma unroll
        for (int ks = 0; ks < kEmbK; ++ks) {
            if (ks < nk) {
                const float a = xr[2 * ks];
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wl[ct][ks], acc[ct], 0, 0, 0);
            }
        }
        if (__builtin_amdgcn_ballot_w64((ms[rt * 32 + j] & 2) != 0) != 0) {   // some token of this tile is conditioned
            const float* cr = cs + (rt * 32 + j) * kEmbLd + hh;
#pragma unroll
            for (int ks = 0; ks < kEmbK; ++ks) {
                if (ks < nk) {
                    const float a = cr[2 * ks];
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wc[ct][ks], acc[ct], 0, 0, 0);
                }
            }
        }
        // epilogue: register r of lane-half hh is token row mfma_row(r, hh) of the tile, lane j its channel
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 4) {
            float add[4][3];
            int mrow[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int tk = rt * 32 + mfma_row(r0 + u, hh);
                mrow[u] = ms[tk];
                const int op = tpos[tk], oi = tipa[tk];
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) {
                    const int c = 96 * w + 32 * ct + j;
                    float v = 0.f;
                    if (POS) v += p.pos_embed[op + c];
                    if (IPA) v += p.ipa_out[oi + c];
                    add[u][ct] = v;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long t = tok0 + rt * 32 + mfma_row(r0 + u, hh);
                if (t < p.N) {
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct)
                        p.h[t * kC + 96 * w + 32 * ct + j] = acc[ct][r0 + u] + b0[ct] + ((mrow[u] & 1) ? me1[ct] : me0[ct]) + add[u][ct];
                }
            }
        }
    }
}

// 16-byte accesses (16-byte aligned buffers); the last n % 4 elements one thread each.  In place: each element is read before it is
// written, by the same thread.
__global__ __launch_bounds__(256) void k_rk_update(const RkState st, long n) {
    const long n4 = n >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = reinterpret_cast<const float4*>(st.y)[i];
        const float4 k0 = st.nk > 0 ? reinterpret_cast<const float4*>(st.k[0])[i] : z;
        const float4 k1 = st.nk > 1 ? reinterpret_cast<const float4*>(st.k[1])[i] : z;
        const float4 k2 = st.nk > 2 ? reinterpret_cast<const float4*>(st.k[2])[i] : z;
        const float4 k3 = st.nk > 3 ? reinterpret_cast<const float4*>(st.k[3])[i] : z;
        reinterpret_cast<float4*>(st.y)[i] = make_float4(rk_state(st, a.x, k0.x, k1.x, k2.x, k3.x), rk_state(st, a.y, k0.y, k1.y, k2.y, k3.y),
                                                         rk_state(st, a.z, k0.z, k1.z, k2.z, k3.z), rk_state(st, a.w, k0.w, k1.w, k2.w, k3.w));
    }
    const long r = (n4 << 2) + i;
    if (i < (n & 3)) {
        float k[kRkMaxK];
#pragma unroll
        for (int j = 0; j < kRkMaxK; ++j) k[j] = j < st.nk ? st.k[j][r] : 0.f;
        st.y[r] = rk_state(st, st.y[r], k[0], k[1], k[2], k[3]);
    }
}

void launch_rk_embed(const EmbedParams& p, const RkState& st, hipStream_t s) {
    const dim3 b(256);
    if ((p.N + 127) / 128 >= 384) {
        const dim3 g((unsigned)((p.N + 127) / 128));
        if (p.pos_embed && p.ipa_out) hipLaunchKernelGGL((k_rk_embed<true, true, 128>), g, b, 0, s, p, st);
        else if (p.pos_embed) hipLaunchKernelGGL((k_rk_embed<true, false, 128>), g, b, 0, s, p, st);
        else if (p.ipa_out) hipLaunchKernelGGL((k_rk_embed<false, true, 128>), g, b, 0, s, p, st);
        else hipLaunchKernelGGL((k_rk_embed<false, false, 128>), g, b, 0, s, p, st);
    } else {
        const dim3 g((unsigned)((p.N + 31) / 32));
        if (p.pos_embed && p.ipa_out) hipLaunchKernelGGL((k_rk_embed<true, true, 32>), g, b, 0, s, p, st);
        else if (p.pos_embed) hipLaunchKernelGGL((k_rk_embed<true, false, 32>), g, b, 0, s, p, st);
        else if (p.ipa_out) hipLaunchKernelGGL((k_rk_embed<false, true, 32>), g, b, 0, s, p, st);
        else hipLaunchKernelGGL((k_rk_embed<false, false, 32>), g, b, 0, s, p, st);
    }
}

void launch_rk_update(const RkState& st, long n, hipStream_t s) {
    const long n4 = n >> 2;
    const long nb = (n4 + 255) / 256;
    hipLaunchKernelGGL(k_rk_update, dim3((unsigned)(nb > 0 ? nb : 1)), dim3(256), 0, s, st, n);
}

}  // namespace mdg
