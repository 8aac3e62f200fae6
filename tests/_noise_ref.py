"""The statement the noise kernel is held to (csrc/kernel_noise.hpp, include/hipfeat.h), in plain numpy: Philox4x32-10 on uint64
arithmetic and the Box-Muller map in float64 (``normals``), and the same map evaluated in numpy float32 (``ref32``)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words; key: two 32-bit words -> the four output words (uint64 arrays)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _words(seed, key, cols):
    """The words behind samples 0 ... cols - 1 of a row: (r, r') per sample, r feeding u1 and r' feeding u2."""
    q = np.arange((cols + 3) // 4, dtype=np.uint64)
    key = int(key) & (2**64 - 1)
    r = philox4x32_10((q & MASK, q >> np.uint64(32), np.full_like(q, key & 0xFFFFFFFF), np.full_like(q, key >> 32)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    ra = np.stack([r[0], r[0], r[2], r[2]], axis=1).reshape(-1)[:cols]
    rb = np.stack([r[1], r[1], r[3], r[3]], axis=1).reshape(-1)[:cols]
    return ra, rb


def normals(seed, key, cols, dtype=np.float64):
    """n(seed, key, t) for t < cols; ``dtype=np.float32`` evaluates the same formulae in float32 (ref32)."""
    ra, rb = _words(seed, key, cols)
    f = dtype
    u1 = ((ra >> np.uint64(8)) + np.uint64(1)).astype(f) * f(2.0**-24)
    u2 = (rb >> np.uint64(8)).astype(f) * f(2.0**-24)
    rad = np.sqrt(f(-2.0) * np.log(u1))
    ang = f(2.0 * np.pi) * u2
    return np.where(np.arange(cols) % 2 == 0, rad * np.cos(ang), rad * np.sin(ang)).astype(f)


def batch(seed, keys, cols, dtype=np.float64):
    return np.stack([normals(seed, k, cols, dtype) for k in keys]) if len(keys) else np.zeros((0, cols), dtype)
