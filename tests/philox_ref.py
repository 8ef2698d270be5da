"""Numpy restatement of the SDE sampler's noise generator (include/mdgen_amd.h, mdgen_sample_sde_rng): the Philox4x32-10 words,
the two uniforms and the deviate in fp64.  Written from the header's description and Random123's known answers, not from
csrc/philox.h or mdgen_amd/philox.py; tests/test_sde_rng_cpu.py holds all three against each other."""
import numpy as np

MUL = (0xD2511F53, 0xCD9E8D57)
WEYL = (0x9E3779B9, 0xBB67AE85)
TWO_PI_F32 = float(np.float32(6.2831855))   # the header's fl(2 pi)


def _mulhilo(m, x):
    p = np.uint64(m) * x.astype(np.uint64)
    return (p >> np.uint64(32)).astype(np.uint32), (p & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def philox(ctr, key):
    """ctr (..., 4) uint32, key (2,) uint32-valued -> (..., 4) uint32."""
    ctr = np.asarray(ctr, dtype=np.uint32)
    c = [ctr[..., i].copy() for i in range(4)]
    k = [int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF]
    for r in range(10):
        if r:
            k = [(k[0] + WEYL[0]) & 0xFFFFFFFF, (k[1] + WEYL[1]) & 0xFFFFFFFF]
        hi0, lo0 = _mulhilo(MUL[0], c[0])
        hi1, lo1 = _mulhilo(MUL[1], c[2])
        c = [hi1 ^ c[1] ^ np.uint32(k[0]), lo1, hi0 ^ c[3] ^ np.uint32(k[1]), lo0]
    return np.stack(c, -1)


def counters(shape, step, block, sample_base=0):
    """(B, T, L, D, 4) uint32: ((t L + l) D + d, sample_base + b, step, block), every word mod 2^32."""
    B, T, L, D = shape
    n = T * L * D
    ctr = np.empty((B, n, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(n, dtype=np.uint64).astype(np.uint32)[None, :]
    ctr[..., 1] = ((np.arange(B, dtype=np.uint64) + np.uint64(sample_base % 2 ** 32)) % np.uint64(2 ** 32)).astype(np.uint32)[:, None]
    ctr[..., 2] = np.uint32(step % 2 ** 32)
    ctr[..., 3] = np.uint32(block % 2 ** 32)
    return ctr.reshape(B, T, L, D, 4)


def key_of(seed):
    seed %= 2 ** 64
    return (seed & 0xFFFFFFFF, seed >> 32)


def uniforms(w):
    """The words (..., 4) -> u1 in (0, 1), u2 in [0, 1) as fp64 (both exactly representable in fp32)."""
    u1 = ((w[..., 0] >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (w[..., 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normal(w):
    """z = sqrt(-2 ln u1) cos(fl(2 pi) u2) in fp64."""
    u1, u2 = uniforms(w)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI_F32 * u2)


def noise(shape, seed, step, block=0, sample_base=0):
    """xi (B, T, L, D) in fp64 and the words behind it."""
    w = philox(counters(shape, step, block, sample_base), key_of(seed))
    return normal(w), w
