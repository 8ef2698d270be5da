// state_embed.h -- the two device bodies that the fixed-grid samplers' state kernels share (k_rk.hip: the Runge-Kutta states,
// k_sde.hip: the SDE states):
//   state_embed   the token embedding (k_embed, k_small.hip) of a state that exists only inside the launch: the staging prologue forms
//                 the token's D values from y and up to NOPS read-only operands (velocities, noise) with the caller's `value`,
//                 stages them in LDS and embeds them; a storing state is also written over y.
//   state_update  the same arithmetic without the embedding, elementwise over n values.
// `value(y, o, e)` is called with the element of y and of every operand (0 where `ops[j]` is null) and the element's flat index e
// in y (k_sde.hip generates its noise there; k_rk.hip ignores it); what it computes, and in which order it rounds, belongs to the
// caller -- this file holds no arithmetic on the state.
#pragma once
#include "kernels.h"

#pragma clang fp contract(off)

namespace mdg {

// k_embed's tile geometry (k_small.hip): 29-float LDS rows, 14 k-steps of v_mfma_f32_32x32x2_f32, the packed B operands of
// launch_pack_embed; workgroups of 128 tokens, or of 32 for the small launches.
constexpr int kEmbLd = 29, kEmbK = 14;
template <bool POS, bool IPA, int kEmbTok, int NOPS, class Value>
__device__ __forceinline__ void state_embed(const EmbedParams& p, float* y, int store, const float* const (&ops)[NOPS], Value value) {
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
    {   // stage the state / x_cond rows: unconditional clamped loads of y, the operands and x_cond, all in flight together
        constexpr int NIT = (kEmbTok * 28 + 255) / 256;
        float a[NIT], b[NIT], kv[NIT][NOPS];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i0 = tid + 256 * it;
            const int i = i0 < kEmbTok * 28 ? i0 : kEmbTok * 28 - 1;
            const int tk = i / 28, d = i % 28;
            long t = tok0 + tk;
            t = t < p.N ? t : p.N - 1;
            const int dc = d < p.D ? d : 0;
            const long e = t * p.D + dc;
            a[it] = y[e];
            b[it] = p.x_cond[e];
#pragma unroll
            for (int j = 0; j < NOPS; ++j) kv[it][j] = ops[j] ? ops[j][e] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + 256 * it;
            if (i >= kEmbTok * 28) break;
            const int tk = i / 28, d = i % 28;
            const bool ok = tok0 + tk < p.N && d < p.D;
            const float v = value(a[it], kv[it], (tok0 + tk) * p.D + d);   // (an index past the state: its value is discarded below)
            xs[tk * kEmbLd + d] = ok ? v : 0.f;
            cs[tk * kEmbLd + d] = ok ? b[it] : 0.f;
            if (ok && b[it] != 0.f) atomicOr(&ms[tk], 2);
            // the state over y: element (token, d) is read and written by this thread alone (the clamped loads of other threads are discarded)
            if (store && ok) y[(tok0 + tk) * p.D + d] = v;
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
template <int NOPS, class Value>
__device__ __forceinline__ void state_update(float* y, const float* const (&ops)[NOPS], long n, Value value) {
    const long n4 = n >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = reinterpret_cast<const float4*>(y)[i];
        float4 k[NOPS];
#pragma unroll
        for (int j = 0; j < NOPS; ++j) k[j] = ops[j] ? reinterpret_cast<const float4*>(ops[j])[i] : z;
        float ox[NOPS], oy[NOPS], oz[NOPS], ow[NOPS];
#pragma unroll
        for (int j = 0; j < NOPS; ++j) { ox[j] = k[j].x; oy[j] = k[j].y; oz[j] = k[j].z; ow[j] = k[j].w; }
        const long e = i << 2;
        reinterpret_cast<float4*>(y)[i] = make_float4(value(a.x, ox, e), value(a.y, oy, e + 1), value(a.z, oz, e + 2), value(a.w, ow, e + 3));
    }
    const long r = (n4 << 2) + i;
    if (i < (n & 3)) {
        float k[NOPS];
#pragma unroll
        for (int j = 0; j < NOPS; ++j) k[j] = ops[j] ? ops[j][r] : 0.f;
        y[r] = value(y[r], k, r);
    }
}

// the launch sizes of launch_embed (k_small.hip): 128-token workgroups from 384 of them on, else 32-token ones
#define MDG_LAUNCH_STATE_EMBED(KERNEL, p, st, s)                                                                      \
    do {                                                                                                              \
        const dim3 b_(256);                                                                                           \
        if (((p).N + 127) / 128 >= 384) {                                                                             \
            const dim3 g_((unsigned)(((p).N + 127) / 128));                                                           \
            if ((p).pos_embed && (p).ipa_out) hipLaunchKernelGGL((KERNEL<true, true, 128>), g_, b_, 0, s, p, st);     \
            else if ((p).pos_embed) hipLaunchKernelGGL((KERNEL<true, false, 128>), g_, b_, 0, s, p, st);              \
            else if ((p).ipa_out) hipLaunchKernelGGL((KERNEL<false, true, 128>), g_, b_, 0, s, p, st);                \
            else hipLaunchKernelGGL((KERNEL<false, false, 128>), g_, b_, 0, s, p, st);                                \
        } else {                                                                                                      \
            const dim3 g_((unsigned)(((p).N + 31) / 32));                                                             \
            if ((p).pos_embed && (p).ipa_out) hipLaunchKernelGGL((KERNEL<true, true, 32>), g_, b_, 0, s, p, st);      \
            else if ((p).pos_embed) hipLaunchKernelGGL((KERNEL<true, false, 32>), g_, b_, 0, s, p, st);               \
            else if ((p).ipa_out) hipLaunchKernelGGL((KERNEL<false, true, 32>), g_, b_, 0, s, p, st);                 \
            else hipLaunchKernelGGL((KERNEL<false, false, 32>), g_, b_, 0, s, p, st);                                 \
        }                                                                                                             \
    } while (0)

}  // namespace mdg
