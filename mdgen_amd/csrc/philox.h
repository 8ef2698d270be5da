// philox.h -- the counter-based generator behind the SDE sampler's in-kernel noise (k_sde.hip), host and device, plain C++.
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers are
// tests/test_sde_rng_cpu.py's): a keyed bijection of a 128-bit counter, so a value needs no memory and no state -- it is a function
// of its coordinates.  The counter layout of one normal deviate is stated in include/mdgen_amd.h (mdgen_sample_sde_rng).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MDG_PHILOX_HD __host__ __device__
#else
#define MDG_PHILOX_HD
#endif

namespace mdg {

// out = Philox4x32-10(ctr; key).  Each round forms its two high / low halves from ONE 64-bit product per multiplier
// (v_mad_u64_u32 on CDNA, where a 32 x 32 multiply is not full rate).
MDG_PHILOX_HD inline void philox4x32_10(const uint32_t (&ctr)[4], const uint32_t (&key)[2], uint32_t (&out)[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;   // the Weyl sequence of the key (the bump after the last round is unused)
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// One standard normal deviate from the first two output words (Box-Muller, the cosine branch), every operation one rounded fp32
// operation with the accurate math functions:
//   u1 = ((w0 >> 9) + 0.5) * 2^-23   exact; in (0, 1), at least 2^-24, so |z| <= 5.77
//   u2 = (w1 >> 8) * 2^-24           exact; in [0, 1)
//   z  = sqrtf(-2 * logf(u1)) * cosf(fl(2 pi) * u2)
MDG_PHILOX_HD inline float philox_normal(uint32_t w0, uint32_t w1) {
    const float u1 = ((float)(w0 >> 9) + 0.5f) * 0x1p-23f;
    const float u2 = (float)(w1 >> 8) * 0x1p-24f;
    return sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
}

// The deviate at (element within the sample, sample, stochastic step, block) under `seed`: key = {low word, high word}
MDG_PHILOX_HD inline float philox_normal_at(uint64_t seed, uint32_t element, uint32_t sample, uint32_t step, uint32_t block) {
    const uint32_t ctr[4] = {element, sample, step, block}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    return philox_normal(w[0], w[1]);
}

}  // namespace mdg
