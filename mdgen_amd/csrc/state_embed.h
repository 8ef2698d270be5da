// state_embed.h -- the two device bodies that the token-embedding kernel and the fixed-grid samplers' state kernels share (k_small.hip:
// k_embed; k_rk.hip: the Runge-Kutta states; k_sde.hip: the SDE states), and their launch sizes:
//   state_embed   the token embedding of a state.  The staging prologue forms the token's D values from y and up to NOPS read-only
//                 operands (velocities, noise) with the caller's `value`, stages them in LDS and embeds them; with `store` the values
//                 are also written there (the samplers pass y itself: the state is updated in place).  k_embed is this body on p.x
//                 with the identity for `value` and no store; a sampler's state exists only inside its launch.
//   state_update  the same arithmetic without the embedding, elementwise over n values.
// `value(y, o, e)` is called with the element of y and of every operand (0 where `ops[j]` is null) and the element's flat index e
// in y (k_sde.hip generates its noise there; k_rk.hip ignores it); what it computes, and in which order it rounds, belongs to the
// caller -- this file holds no arithmetic on the state, and including it leaves the includer's floating-point mode as it was (the
// bodies switch contraction off for themselves).
#pragma once
#include <type_traits>
#include "kernels.h"

namespace mdg {

// -------------------------------------------------------------------------------------------------
// Token embedding (latent_model.py:233-246):
//   h = latent_to_emb(x) [+ pos_embed[l]] + cond_to_emb(x_cond) + mask_to_emb[x_cond_mask] + ipa_out[b,l]
// A [N x D] . [D x 384] product with D = 21 / 28: far too thin for the bf16 path's panels, and as a per-channel dot
// product on the VALU (round 1) it ran at 0.9 TB/s of its 98 MB output.  Here it is an fp32 MFMA job:
// v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate -- the reference's arithmetic), D = tokens x channels.
// Workgroup = 128 tokens (4 row tiles) x 384 channels; wave w owns channels 96 w .. 96 w + 95 and keeps its slices
// of both weight matrices in registers (2 x 3 tiles x 14 k-steps); token rows are staged once in LDS (row stride 29
// floats: the per-k column reads are conflict-free).  cond_to_emb is skipped for row tiles whose x_cond rows are all
// zero (every non-conditioning frame).  The epilogue adds bias, mask embedding, pos_embed / ipa_out rows (requested
// four token rows ahead) and stores 128-byte row segments.
// -------------------------------------------------------------------------------------------------
// The tile geometry: 29-float LDS rows, 14 k-steps, the packed B operands of launch_pack_embed.
constexpr int kEmbLd = 29, kEmbK = 14;
// POS / IPA: pos_embed / ipa_out present (compile-time so that their loads are unconditional).
// kEmbTok: tokens per workgroup -- 128 when that still makes a few hundred workgroups; 32 (one row tile per workgroup) for the
// small launches (B = 1, the TPS shard), whose time is one workgroup's latency: 40 -> ~17 us at 12 800 tokens.
template <bool POS, bool IPA, int kEmbTok, int NOPS, class Value>
__device__ __forceinline__ void state_embed(const EmbedParams& p, const float* y, float* store, const float* const (&ops)[NOPS], Value value) {
#pragma clang fp contract(off)
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
            const int i = i0 < kEmbTok * 28 ? i0 : kEmbTok * 28 - 1;   // (32-token workgroups: 3.5 rounds)
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
            // in place (store == y): element (token, d) is read and written by this thread alone (the clamped loads of other threads are discarded)
            if (store && ok) store[(tok0 + tk) * p.D + d] = v;
        }
    }
    const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id(), hh = lane >> 5, j = lane & 31;
    const int nk = (p.D + 1) >> 1;
    // B operands (k = 2 ks + hh, column = channel): this wave's three channel tiles of both weight matrices
    // (from the packed copies, k_pack_embed: one 256-byte request per (tile, k-step) instead of 64 lines 84 bytes apart --
    // 168 such gathers per lane were the fixed cost of every workgroup)
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
#pragma clang fp contract(off)
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

// state_update's grid: one thread per 16 bytes, at least one workgroup (for the last n % 4 elements)
inline dim3 state_update_grid(long n) {
    const long nb = ((n >> 2) + 255) / 256;
    return dim3((unsigned)(nb > 0 ? nb : 1));
}

// The kernel form and grid of an embedding launch, chosen once for k_embed and the state kernels: 128-token workgroups from 384 of
// them on, else 32-token ones.  `launch(pos, ipa, tok, grid)` gets POS, IPA and kEmbTok as std::integral_constants.
template <class Launch>
void embed_dispatch(const EmbedParams& p, Launch launch) {
    const bool big = (p.N + 127) / 128 >= 384;
    const dim3 g((unsigned)(big ? (p.N + 127) / 128 : (p.N + 31) / 32));
    auto with_ipa = [&](auto pos, auto ipa) {
        if (big) launch(pos, ipa, std::integral_constant<int, 128>{}, g);
        else launch(pos, ipa, std::integral_constant<int, 32>{}, g);
    };
    auto with_pos = [&](auto pos) {
        if (p.ipa_out) with_ipa(pos, std::true_type{});
        else with_ipa(pos, std::false_type{});
    };
    if (p.pos_embed) with_pos(std::true_type{});
    else with_pos(std::false_type{});
}

}  // namespace mdg
