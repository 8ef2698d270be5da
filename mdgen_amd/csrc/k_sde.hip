// k_sde.hip -- the device side of the SDE sampler (sde.inc: Euler-Maruyama and Heun on t = linspace(t0, t1, n_points)).
//   k_sde_embed   state_embed.h's embedding of an SDE state (SdeForm, kernels.h) formed from x, up to two velocities and the step's
//                 noise: the first launch of step i forms the result of step i - 1 (for Heun with step i's noise term added) and
//                 stores it over x; Heun's predictor exists only inside its launch.
//   k_sde_update  the same arithmetic without the embedding: the last step (Mean / Tweedie / Euler), or the result of the last
//                 stochastic step when there is none.
// Each has a second instantiation that computes the step's noise with philox.h at the element's coordinates instead of reading it.
// The formulas are the reference's integrators.py:26-45 and transport.py:306-345, restated in sde.inc.  Every written operation is one
// rounded fp32 operation and nothing is contracted into an FMA; the coefficients come from the host, so the device never divides.
#include "philox.h"
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

// The generated noise (philox.h; the counter layout is include/mdgen_amd.h's): the seed words are read from device memory here, in
// the kernel -- never baked into its arguments -- so a replayed graph draws what the buffer holds at replay.
struct SdeRng {
    uint64_t seed;
    uint32_t sample0, step, block, per_b;   // counter words c1 (of the launch's first sample), c2, c3; elements of one sample
};
__device__ __forceinline__ SdeRng sde_rng_of(const SdeState& s) {
    SdeRng g;
    g.seed = s.rng[0];
    g.sample0 = (uint32_t)s.rng[1] + (uint32_t)s.b0;
    g.step = (uint32_t)s.step;
    g.block = (uint32_t)s.rng[2] + (uint32_t)s.block;
    g.per_b = s.per_b;
    return g;
}
// xi at flat index e of the launch's state: sample e / per_b of the launch, element e % per_b of that sample
__device__ __forceinline__ float sde_noise(const SdeRng& g, long e) {
    uint32_t b, el;
    if ((unsigned long)e >> 32) {
        b = (uint32_t)((unsigned long)e / g.per_b);
        el = (uint32_t)((unsigned long)e % g.per_b);
    } else {
        b = (uint32_t)e / g.per_b;
        el = (uint32_t)e - b * g.per_b;
    }
    return philox_normal_at(g.seed, el, g.sample0 + b, g.step, g.block);
}

// RNG: the noise-reading forms take xi from the generator, not from st.xi; the arithmetic on it is the same sde_state
template <bool RNG, bool POS, bool IPA, int kEmbTok>
__device__ __forceinline__ void sde_embed(const EmbedParams& p, const SdeState& st) {
    const float* const ops[3] = {st.v[0], st.v[1], RNG ? nullptr : st.xi};
    float* const store = st.store ? st.y : nullptr;
    if constexpr (RNG) {
        const SdeRng g = sde_rng_of(st);
        state_embed<POS, IPA, kEmbTok>(p, st.y, store, ops, [&](float x, const float* o, long e) { return sde_state(st, x, o[0], o[1], sde_noise(g, e)); });
    } else {
        state_embed<POS, IPA, kEmbTok>(p, st.y, store, ops, [&](float x, const float* o, long) { return sde_state(st, x, o[0], o[1], o[2]); });
    }
}
template <bool POS, bool IPA, int kEmbTok>
__global__ __launch_bounds__(256) void k_sde_embed(const EmbedParams p, const SdeState st) {
    sde_embed<false, POS, IPA, kEmbTok>(p, st);
}
template <bool POS, bool IPA, int kEmbTok>
__global__ __launch_bounds__(256) void k_sde_embed_rng(const EmbedParams p, const SdeState st) {
    sde_embed<true, POS, IPA, kEmbTok>(p, st);
}

template <bool RNG>
__global__ __launch_bounds__(256) void k_sde_update(const SdeState st, long n) {
    const float* const ops[3] = {st.v[0], st.v[1], RNG ? nullptr : st.xi};
    if constexpr (RNG) {
        const SdeRng g = sde_rng_of(st);
        state_update(st.y, ops, n, [&](float x, const float* o, long e) { return sde_state(st, x, o[0], o[1], sde_noise(g, e)); });
    } else {
        state_update(st.y, ops, n, [&](float x, const float* o, long) { return sde_state(st, x, o[0], o[1], o[2]); });
    }
}

// (only a noise-reading state carries st.rng: sde.inc with_noise)
void launch_sde_embed(const EmbedParams& p, const SdeState& st, hipStream_t s) {
    embed_dispatch(p, [&](auto pos, auto ipa, auto tok, dim3 g) {
        constexpr bool POS = decltype(pos)::value, IPA = decltype(ipa)::value;
        constexpr int kEmbTok = decltype(tok)::value;
        if (st.rng) hipLaunchKernelGGL((k_sde_embed_rng<POS, IPA, kEmbTok>), g, dim3(256), 0, s, p, st);
        else hipLaunchKernelGGL((k_sde_embed<POS, IPA, kEmbTok>), g, dim3(256), 0, s, p, st);
    });
}

void launch_sde_update(const SdeState& st, long n, hipStream_t s) {
    const dim3 g = state_update_grid(n);
    if (st.rng) hipLaunchKernelGGL(k_sde_update<true>, g, dim3(256), 0, s, st, n);
    else hipLaunchKernelGGL(k_sde_update<false>, g, dim3(256), 0, s, st, n);
}

}  // namespace mdg
