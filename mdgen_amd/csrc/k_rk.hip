// k_rk.hip -- the device side of the fixed-grid Runge-Kutta sampler (ode.inc: midpoint, heun3, rk4 on t = linspace(0, 1, S + 1)).
//   k_rk_embed   k_embed's body (state_embed.h) on a state that exists only inside the launch: the staging prologue forms the token's
//                D values from y0 and up to four velocities (RkState), stages them in LDS and embeds them.  The first stage of step
//                i + 1 is the launch that forms y1 of step i: it also stores y1 over y0.
//   k_rk_update  the same arithmetic without the embedding: the result of the last step.
// Both bodies are state_embed.h's (shared with k_small.hip and k_sde.hip); this file holds the arithmetic of the states.
// A network evaluation outside the Euler graph otherwise starts with k_embed reading a state that a separate k_ode_combine launch
// has just written: one launch and one round trip of the state through HBM per evaluation.
// Every written operation of a state is one rounded fp32 operation (the formulas are torchdiffeq's fixed_grid.py / rk_common.py,
// restated in ode.inc): nothing is contracted into an FMA.
#include "state_embed.h"

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

template <bool POS, bool IPA, int kEmbTok>
__global__ __launch_bounds__(256) void k_rk_embed(const EmbedParams p, const RkState st) {
    const float* const ops[kRkMaxK] = {st.nk > 0 ? st.k[0] : nullptr, st.nk > 1 ? st.k[1] : nullptr, st.nk > 2 ? st.k[2] : nullptr,
                                       st.nk > 3 ? st.k[3] : nullptr};
    state_embed<POS, IPA, kEmbTok>(p, st.y, st.store ? st.y : nullptr, ops, [&](float y0, const float* k, long) { return rk_state(st, y0, k[0], k[1], k[2], k[3]); });
}

__global__ __launch_bounds__(256) void k_rk_update(const RkState st, long n) {
    const float* const ops[kRkMaxK] = {st.nk > 0 ? st.k[0] : nullptr, st.nk > 1 ? st.k[1] : nullptr, st.nk > 2 ? st.k[2] : nullptr,
                                       st.nk > 3 ? st.k[3] : nullptr};
    state_update(st.y, ops, n, [&](float y0, const float* k, long) { return rk_state(st, y0, k[0], k[1], k[2], k[3]); });
}

void launch_rk_embed(const EmbedParams& p, const RkState& st, hipStream_t s) {
    embed_dispatch(p, [&](auto pos, auto ipa, auto tok, dim3 g) {
        hipLaunchKernelGGL((k_rk_embed<decltype(pos)::value, decltype(ipa)::value, decltype(tok)::value>), g, dim3(256), 0, s, p, st);
    });
}

void launch_rk_update(const RkState& st, long n, hipStream_t s) {
    hipLaunchKernelGGL(k_rk_update, state_update_grid(n), dim3(256), 0, s, st, n);
}

}  // namespace mdg
