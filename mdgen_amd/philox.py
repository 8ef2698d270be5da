"""The SDE sampler's generated noise on the host: a numpy restatement of csrc/philox.h and of the counter layout stated in
include/mdgen_amd.h (mdgen_sample_sde_rng).  `Sampler.sample_sde`'s host loop over a generic callable draws from it, so that
loop and the library's kernels integrate the same noise (to the rounding of logf / cosf: the words and u1, u2 are exact).
`bridge_uniform` is the uniform of the transition-path sampler (mdgen_tp_sample, csrc/k_tps.hip), exact as well."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counter words under the key words: broadcastable integer arrays -> four uint32 arrays."""
    c = [np.asarray(v).astype(np.uint64) & _MASK for v in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(np.broadcast_arrays(*[v.astype(np.uint32) for v in c]))


def normal(w0, w1):
    """The deviate of the first two output words, in fp32 as csrc/philox.h writes it."""
    f = np.float32
    u1 = ((w0 >> np.uint32(9)).astype(f) + f(0.5)) * f(2.0 ** -23)
    u2 = (w1 >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    return (np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(6.2831855) * u2)).astype(f)


def sde_noise(shape, seed, step, block_base=0, sample_base=0, block=0):
    """xi (B, T, L, D) fp32 of stochastic step `step` of block `block`: element (b, t, l, d) at the counter ((t L + l) D + d,
    sample_base + b, step, block_base + block) under the key {seed low word, seed high word}."""
    B, T, L, D = (int(v) for v in shape)
    if T * L * D >= 1 << 32:
        raise ValueError("T * L * D does not fit the generator's 32-bit element counter")
    seed = int(seed) % (1 << 64)
    el = np.arange(T * L * D, dtype=np.uint64)[None, :]
    b = ((np.arange(B, dtype=np.uint64) + np.uint64(int(sample_base) % (1 << 32))) & _MASK)[:, None]
    w = philox4x32_10(el, b, int(step) % (1 << 32), (int(block_base) + int(block)) % (1 << 32), seed & 0xFFFFFFFF, seed >> 32)
    return normal(w[0], w[1]).reshape(B, T, L, D)


def bridge_uniform(seed, stream, sample, t):
    """u fp64 in [0, 1) of the bridge sampler (include/mdgen_amd.h mdgen_tp_sample) for path `sample` (a 64-bit index:
    sample_base + the position in the call) at step `t`, both broadcastable integer arrays: the words x0, x1 at the counter
    (sample low word, sample high word, t, stream) under the key {seed low word, seed high word};
    u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53, 53 bits, exact."""
    seed = int(seed) % (1 << 64)
    sample = np.asarray(sample).astype(np.uint64)
    w = philox4x32_10(sample & _MASK, sample >> np.uint64(32), np.asarray(t).astype(np.uint64) & _MASK, int(stream) % (1 << 32),
                      seed & 0xFFFFFFFF, seed >> 32)
    hi, lo = (w[0] >> np.uint32(5)).astype(np.uint64), (w[1] >> np.uint32(6)).astype(np.uint64)
    return ((hi << np.uint64(26)) + lo).astype(np.float64) * 2.0 ** -53
