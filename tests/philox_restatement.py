"""Test helper: a numpy restatement of the library's device RNG (csrc/philox.h) -- Philox4x32-10 with the Random123 constants, the
counter layout (block_lo, block_hi, draw_lo, draw_hi) under the 64-bit seed as key, the fp32 construction of Box-Muller's u and v,
and the transform itself in float64 from those fp32 values (so the device's fp32 logf / sqrtf / sinf / cosf are measured against a
reference that is exact to fp32's eyes).  Written from the published algorithm (Salmon et al., SC'11), not from the kernel.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                    # 32 x 32 -> 64 bit products (no overflow in uint64)
        hi0, lo0, hi1, lo1 = p0 >> SH, p0 & MASK, p1 >> SH, p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def blocks(seed, draw, n_blocks, first_block=0):
    """the words [n_blocks, 4] of blocks first_block .. of draw `draw` of the stream `seed`"""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    b = np.arange(first_block, first_block + n_blocks, dtype=np.uint64)
    ones = np.ones(n_blocks, dtype=np.uint64)
    w = philox4x32_10([b & MASK, b >> SH, ones * np.uint64(draw & 0xFFFFFFFF), ones * np.uint64(draw >> 32)],
                      (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1)


def u32(seed, draw, n):
    """the first n words of a draw: element e is lane e % 4 of block e // 4"""
    return blocks(seed, draw, (n + 3) // 4).reshape(-1)[:n]


def box_muller_inputs(w0, w1):
    """(u, v) as the device forms them, in fp32: u = w0 2^-32 + 2^-33 (the product is exact; one rounding in the sum), v = w1 (2 pi 2^-32)"""
    u = w0.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)
    v = w1.astype(np.float32) * np.float32(np.float32(6.28318530717958647692) * np.float32(2.0 ** -32))
    assert u.dtype == np.float32 and v.dtype == np.float32
    return u, v


def randn(seed, draw, n):
    """float64 [n]: Box-Muller in float64 from the fp32 (u, v); lanes 0/1 = r cos v, r sin v from (w0, w1), lanes 2/3 from (w2, w3)"""
    w = blocks(seed, draw, (n + 3) // 4)
    out = np.empty((w.shape[0], 4), dtype=np.float64)
    for p in range(2):
        u, v = box_muller_inputs(w[:, 2 * p], w[:, 2 * p + 1])
        u, v = u.astype(np.float64), v.astype(np.float64)
        r = np.sqrt(-2.0 * np.log(u))
        out[:, 2 * p], out[:, 2 * p + 1] = r * np.cos(v), r * np.sin(v)
    return out.reshape(-1)[:n]


def moment_checks(z, z_next):
    """The statistical asserts of the RNG tests, shared by the device test and the CPU check of the restatement itself.  z, z_next:
    two successive draws of N normals.  Every margin is 5 standard errors of the estimator under N(0, 1), from N alone."""
    z, z_next = np.asarray(z, dtype=np.float64), np.asarray(z_next, dtype=np.float64)
    N = z.size
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2 - 3.0
    corr_draw = np.corrcoef(z, z_next)[0, 1]
    corr_nb = np.corrcoef(z[:-1], z[1:])[0, 1]
    got = dict(mean=mean, var=var, kurt=kurt, corr_draw=corr_draw, corr_nb=corr_nb)
    assert abs(mean) <= 5 / np.sqrt(N), got
    assert abs(var - 1) <= 5 * np.sqrt(2 / N), got
    assert abs(kurt) <= 5 * np.sqrt(24 / N), got
    assert abs(corr_draw) <= 5 / np.sqrt(N), got
    assert abs(corr_nb) <= 5 / np.sqrt(N), got
    return got
