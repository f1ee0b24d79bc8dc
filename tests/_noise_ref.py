"""numpy restatement of the receiver-noise contract (include/gpsiq.h, "receiver noise"), independent of the library: the knots come
from scripts/gen_noise_knots.py's formulas (statistics.NormalDist), the generator is written out here in uint64 arithmetic.
Vectorised over the 64 x nblocks lane streams, one row at a time."""
import math
import statistics

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
MUL = np.uint64(0x5851F42D4C957F2D)
INC = np.uint64(0x14057B7EF767814F)


def knots():
    inv = statistics.NormalDist().inv_cdf
    K = np.array([round(4096.0 * inv(0.5 + (64 * k + 0.5) / 65536.0)) for k in range(512)], dtype=np.int64)
    T = np.array([round(4096.0 * inv(0.5 + (32704 + f + 0.5) / 65536.0)) for f in range(64)], dtype=np.int64)
    return K, T


def unscaled_magnitudes(K, T):
    m = np.arange(32768)
    k, f = m >> 6, m & 63
    kk = np.minimum(k, 510)
    seg = K[kk] + (((K[kk + 1] - K[kk]) * f) >> 6)
    return np.where(k < 511, seg, T[f])


def scale_c():
    K, T = knots()
    mag = unscaled_magnitudes(K, T).astype(np.float64) / 4096.0
    return 1.0 / math.sqrt(float(np.mean(mag * mag)))


def tables(sigma):
    K, T = knots()
    s = sigma * scale_c()
    S = np.rint(s * K.astype(np.float64) * 2.0 ** -12).astype(np.int64)
    St = np.rint(s * T.astype(np.float64) * 2.0 ** -12).astype(np.int64)
    return S, St


def z_of(u, S, St):
    u = u.astype(np.int64)
    s, m = u >> 15, u & 0x7FFF
    k, f = m >> 6, m & 63
    kk = np.minimum(k, 510)
    mag = np.where(k < 511, S[kk] + (((S[kk + 1] - S[kk]) * f) >> 6), St[f])
    return np.where(s == 1, -mag, mag)


def splitmix64(x):
    with np.errstate(over="ignore"):
        z = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def xsh_rr(x):
    xs = (((x >> np.uint64(18)) ^ x) >> np.uint64(27)) & np.uint64(0xFFFFFFFF)
    rot = x >> np.uint64(59)
    return ((xs >> rot) | (xs << ((np.uint64(32) - rot) & np.uint64(31)))) & np.uint64(0xFFFFFFFF)


def lcg(x, inc=INC):
    with np.errstate(over="ignore"):
        return x * MUL + np.uint64(inc)


def noise(seed, sigma, block0, nblocks, nsamp):
    """int64 array [nblocks, nsamp, 2] of (zI, zQ) for absolute blocks block0 .. block0+nblocks-1."""
    S, St = tables(sigma)
    B = (np.uint64(block0) + np.arange(nblocks, dtype=np.uint64))[:, None]
    lanes = np.arange(64, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = splitmix64(np.uint64(seed) ^ splitmix64(B * np.uint64(64) + lanes))      # [nblocks, 64]
    rows = (nsamp + 63) // 64
    out = np.zeros((nblocks, rows * 64, 2), dtype=np.int64)
    for j in range(rows):
        w = xsh_rr(x)
        out[:, j * 64:(j + 1) * 64, 0] = z_of(w & np.uint64(0xFFFF), S, St)
        out[:, j * 64:(j + 1) * 64, 1] = z_of(w >> np.uint64(16), S, St)
        x = lcg(x)
    return out[:, :nsamp]


def pcg32_srandom(initstate, initseq, count):
    """PCG32 reference seeding (pcg32_srandom_r) and outputs: the known-answer check of the LCG and xsh_rr."""
    inc = (np.uint64(initseq) << np.uint64(1)) | np.uint64(1)
    st = np.uint64(0)
    st = lcg(st, inc)
    with np.errstate(over="ignore"):
        st = st + np.uint64(initstate)
    st = lcg(st, inc)
    out = []
    for _ in range(count):
        out.append(int(xsh_rr(st)))
        st = lcg(st, inc)
    return out


def add_noise16(clean, z):
    """int16 IQ [.., 2*nsamp] + z [.., nsamp, 2], mod 2^16."""
    c = clean.astype(np.int64).reshape(z.shape)
    return ((c + z + 32768) % 65536 - 32768).astype(np.int16).reshape(clean.shape)
