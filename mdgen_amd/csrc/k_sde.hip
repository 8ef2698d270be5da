// k_sde.hip -- the device side of the SDE sampler (sde.inc: Euler-Maruyama and Heun on t = linspace(t0, t1, n_points)).
//   k_sde_embed   state_embed.h's embedding of an SDE state (SdeForm, kernels.h) formed from x, up to two velocities and the step's
//                 noise: the first launch of step i forms the result of step i - 1 (for Heun with step i's noise term added) and
//                 stores it over x; Heun's predictor exists only inside its launch.
//   k_sde_update  the same arithmetic without the embedding: the last step (Mean / Tweedie / Euler), or the result of the last
//                 stochastic step when there is none.
// The formulas are the reference's integrators.py:26-45 and transport.py:306-345, restated in sde.inc.  Every written operation is one
// rounded fp32 operation and nothing is contracted into an FMA; the coefficients come from the host, so the device never divides.
#include "state_embed.h"

#pragma clang fp contract(off)

namespace mdg {

// velocity + diffusion * score at evaluation time j
__device__ __forceinline__ float sde_drift(const SdeState& s, int j, float v, float x) {
    return v + s.D[j] * (((s.R[j] * v) - x) * s.iV[j]);
}

__device__ __forceinline__ float sde_state(const SdeState& s, float x, float v0, float v1, float xi) {
    switch (s.form) {
    case kSdeNoise: return x + s.G * (xi * s.q);
    case kSdeEm: return (x + sde_drift(s, 0, v0, x) * s.dt) + s.G * (xi * s.q);
    case kSdeDrift: return x + s.dt * sde_drift(s, 0, v0, x);
    case kSdeHeun:
    case kSdeHeunNoise: {
        const float k1 = sde_drift(s, 0, v0, x);
        const float xp = x + s.dt * k1;
        const float k2 = sde_drift(s, 1, v1, xp);
        const float r = x + s.hdt * (k1 + k2);
        return s.form == kSdeHeun ? r : r + s.G * (xi * s.q);
    }
    case kSdeTweedie: return x * s.c[0] + s.c[1] * (((s.R[0] * v0) - x) * s.iV[0]);
    case kSdeEuler: return x + v0 * s.dt;
    default: return x;
    }
}

template <bool POS, bool IPA, int kEmbTok>
__global__ __launch_bounds__(256) void k_sde_embed(const EmbedParams p, const SdeState st) {
    const float* const ops[3] = {st.v[0], st.v[1], st.xi};
    state_embed<POS, IPA, kEmbTok>(p, st.y, st.store, ops, [&](float x, const float* o) { return sde_state(st, x, o[0], o[1], o[2]); });
}

__global__ __launch_bounds__(256) void k_sde_update(const SdeState st, long n) {
    const float* const ops[3] = {st.v[0], st.v[1], st.xi};
    state_update(st.y, ops, n, [&](float x, const float* o) { return sde_state(st, x, o[0], o[1], o[2]); });
}

void launch_sde_embed(const EmbedParams& p, const SdeState& st, hipStream_t s) { MDG_LAUNCH_STATE_EMBED(k_sde_embed, p, st, s); }

void launch_sde_update(const SdeState& st, long n, hipStream_t s) {
    const long n4 = n >> 2;
    const long nb = (n4 + 255) / 256;
    hipLaunchKernelGGL(k_sde_update, dim3((unsigned)(nb > 0 ? nb : 1)), dim3(256), 0, s, st, n);
}

}  // namespace mdg
