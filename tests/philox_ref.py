"""Reference for the device's counter-based normal generator (asva_amd/csrc/philox.h, include/avsd.h "random numbers"), in numpy:
Philox4x32-10 as published by Random123 in uint64 arithmetic (exact), and the normals built on it in float64.

    key      = (seed lo, seed hi)
    counter  = (block lo, block hi, step, stream),  block = element index >> 2
    element  = lane (element index & 3) of its block
    lanes 0, 1 = r cos(2 pi v), r sin(2 pi v) with u, v from words 0, 1; lanes 2, 3 the same from words 2, 3
    u = ((w >> 9) + 0.5) 2^-23,  v = (w' >> 8) 2^-24,  r = sqrt(-2 log u)

The uniforms are exact in f32, so the float64 normals here start from exactly the inputs the device's f32 arithmetic starts from."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def block_words(seed, stream, step, first_block, n_blocks):
    """(n_blocks, 4) uint32: the words of blocks first_block .. first_block + n_blocks - 1"""
    seed = int(seed)
    blocks = np.uint64(first_block) + np.arange(n_blocks, dtype=np.uint64)
    w = philox4x32_10((blocks & MASK, blocks >> S32, np.uint64(int(step)), np.uint64(int(stream))), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1)


def words(n, seed, stream=0, step=0, first=0):
    """words first .. first + n - 1 of the sequence, uint32"""
    first, n = int(first), int(n)
    b0, b1 = first >> 2, (first + n - 1) >> 2
    flat = block_words(seed, stream, step, b0, b1 - b0 + 1).reshape(-1)
    return flat[first - 4 * b0:first - 4 * b0 + n]


def normals(n, seed, stream=0, step=0, first=0):
    """normals first .. first + n - 1 of the sequence, float64"""
    first, n = int(first), int(n)
    b0, b1 = first >> 2, (first + n - 1) >> 2
    w = block_words(seed, stream, step, b0, b1 - b0 + 1)
    z = np.empty(w.shape, dtype=np.float64)
    for lane in (0, 2):
        u = ((w[:, lane] >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        v = (w[:, lane + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        z[:, lane], z[:, lane + 1] = r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)
    flat = z.reshape(-1)
    return flat[first - 4 * b0:first - 4 * b0 + n]


def moments(z):
    """standardised mean, variance, excess kurtosis and lag-1 correlation of a sample that should be N(0, 1): each is
    approximately N(0, 1) itself (mean sqrt(n), (var - 1) sqrt(n / 2), kurtosis sqrt(n / 24), correlation sqrt(n))"""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    m, var = z.mean(), z.var()
    kurt = ((z - m) ** 4).mean() / var ** 2 - 3.0
    corr = ((z[:-1] - m) * (z[1:] - m)).mean() / var
    return m * np.sqrt(n), (var - 1.0) * np.sqrt(n / 2.0), kurt * np.sqrt(n / 24.0), corr * np.sqrt(n)
