"""The spectrum stage restated: include/gpsiq_rows.h, "Spectrum", twice -- as an integer matrix product in numpy (what the GPU tests
compare every byte with) and a sample and a bin at a time in Python ints (what the first is held to on the CPU).  The table is the
library's own carrier table (gpsiq.carrier_table()).  TEST INFRASTRUCTURE: nothing here is product code."""
import functools

import numpy as np

import gpsiq
from gpsiq.abi import SC08

U64 = 2 ** 64 - 1
MAX_SHIFT = 40


@functools.lru_cache(maxsize=None)
def table():
    c, s = gpsiq.carrier_table()
    return np.asarray(c, np.int64), np.asarray(s, np.int64)


def full_range(rng, n, sample_size):
    """n complex samples over the whole range of the format, [n, 2]"""
    if sample_size == SC08:
        return rng.integers(-128, 128, size=(n, 2)).astype(np.int8)
    return rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)


def span(nsamp, nfft, hop, navg):
    nseg = 0 if nsamp < nfft else (nsamp - nfft) // hop + 1
    return nseg, nseg // navg


def ymax(sample_size, nfft, window):
    return (4 if window else 1) * nfft * 500 * (128 if sample_size == SC08 else 32768)


def fits(sample_size, nfft, window, navg, shift):
    y = ymax(sample_size, nfft, window)
    ys = y if shift == 0 else (y >> shift) + 1
    return 2 * navg * ys * ys <= U64


def min_shift(sample_size, nfft, window, navg):
    for s in range(MAX_SHIFT + 1):
        if fits(sample_size, nfft, window, navg, s):
            return s
    return None


@functools.lru_cache(maxsize=None)
def twiddles(nfft):
    """(C, S) [bin k][n]: c(idx), s(idx) at idx = (k n T) mod 512"""
    c, s = table()
    k = np.arange(nfft).reshape(-1, 1)
    n = np.arange(nfft).reshape(1, -1)
    idx = (k * n * (512 // nfft)) % 512
    return c[idx], s[idx]


def segments(x, nfft, hop, count):
    x = np.asarray(x).astype(np.int64)
    return np.stack([x[q * hop:q * hop + nfft] for q in range(count)]) if count else np.zeros((0, nfft, 2), np.int64)


def windowed_bins(x, nfft, hop, window, count):
    """Y of the first `count` segments: (Yi, Yq) int64 [count][nfft] (|Y| < 2^36)"""
    seg = segments(x, nfft, hop, count)
    C, S = twiddles(nfft)
    I, Q = seg[:, :, 0], seg[:, :, 1]
    xi = I @ C.T + Q @ S.T
    xq = Q @ C.T - I @ S.T
    if window:
        xi = 2 * xi - np.roll(xi, 1, axis=1) - np.roll(xi, -1, axis=1)
        xq = 2 * xq - np.roll(xq, 1, axis=1) - np.roll(xq, -1, axis=1)
    return xi, xq


def spectrum_ref(x, nfft, hop, window, navg, shift):
    """x [nsamp, 2] int8 / int16 -> power uint64 [ngroups][nfft]; exact: the cells and the sums are checked to stay inside uint64"""
    nseg, ngroups = span(len(x), nfft, hop, navg)
    if ngroups == 0:
        return np.zeros((0, nfft), np.uint64)
    yi, yq = windowed_bins(x, nfft, hop, window, ngroups * navg)
    ai, aq = np.abs(yi >> shift).astype(np.uint64), np.abs(yq >> shift).astype(np.uint64)      # (>> on int64 is arithmetic and floors)
    top = max(int(ai.max()), int(aq.max()))
    assert 2 * top * top <= U64, "a cell would pass 2^64 - 1: the call is outside the contract's bound"
    cells = (ai * ai + aq * aq).reshape(ngroups, navg, nfft)
    if int(cells.max()) * navg <= U64:
        return cells.sum(axis=1, dtype=np.uint64)
    sums = cells.astype(object).sum(axis=1)
    assert max(int(v) for v in sums.ravel()) <= U64
    return sums.astype(np.uint64)


def spectrum_scalar(x, nfft, hop, window, navg, shift, bins):
    """the contract a sample and a bin at a time, Python ints: {(g, k): power} for the bins asked for"""
    c, s = (t.tolist() for t in table())
    x = np.asarray(x).astype(np.int64).tolist()
    T = 512 // nfft
    nseg = 0 if len(x) < nfft else (len(x) - nfft) // hop + 1
    ngroups = nseg // navg

    def X(q, k):
        xi = xq = 0
        for n in range(nfft):
            I, Q = x[q * hop + n]
            idx = (k * n * T) % 512
            xi += I * c[idx & 511] + Q * s[idx & 511]
            xq += Q * c[idx & 511] - I * s[idx & 511]
        return xi, xq

    out = {}
    for g in range(ngroups):
        for k in bins:
            total = 0
            for q in range(g * navg, g * navg + navg):
                yi, yq = X(q, k)
                if window:
                    lo, hi = X(q, (k - 1) % nfft), X(q, (k + 1) % nfft)
                    yi, yq = 2 * yi - lo[0] - hi[0], 2 * yq - lo[1] - hi[1]
                yi, yq = yi >> shift, yq >> shift                     # Python's >> floors
                total += yi * yi + yq * yq
            assert total <= U64
            out[(g, k)] = total
    return out


def adversarial(sample_size, nfft, nseg, hop, k0=1):
    """a span at full scale whose signs are chosen against bin k0's twiddles: every term of Xi[k0] of every segment that
    starts at a multiple of nfft has the same sign (with hop = nfft: all of them)"""
    c, s = table()
    lo = -128 if sample_size == SC08 else -32768
    hi = -lo - 1
    n = np.arange((nseg - 1) * hop + nfft)
    idx = (k0 * (n % nfft) * (512 // nfft)) % 512
    x = np.empty((len(n), 2), np.int64)
    x[:, 0] = np.where(c[idx] < 0, lo, hi)                            # I c(idx) >= 0 and Q s(idx) >= 0 at every sample
    x[:, 1] = np.where(s[idx] < 0, lo, hi)
    return x.astype(np.int8 if sample_size == SC08 else np.int16)


def table_tone(nfft, k0, count, hop, amp_shift=1):
    """a tone built from the table itself turning at +k0 fs / nfft: I = c(idx) >> amp_shift, Q = s(idx) >> amp_shift (int8: |250 >> 1| fits)"""
    c, s = table()
    n = np.arange((count - 1) * hop + nfft)
    idx = (k0 * n * (512 // nfft)) % 512
    return np.stack([c[idx] >> amp_shift, s[idx] >> amp_shift], axis=1).astype(np.int8)
