"""gpsiq_cfilter and gpsiq_notch_find restated from their contract (include/gpsiq_rows.h, "Complex filter and notch"): numpy in int64
for the filter, a scalar statement in Python integers beside it, Python integers for the lines of a spectrum.  TEST INFRASTRUCTURE:
nothing here reads a line of the library.

Streams are integer arrays [n, 2] (I, Q) or flat interleaved [2 n]; taps are [ntaps, 2] (re, im); `head` is the ntaps - 1 samples
before the span or None (zeros)."""
import math
from fractions import Fraction

import numpy as np

from _filter_ref import span, full_range  # noqa: F401  (the span arithmetic and the pools are the filter's)

TAP_SUM = 65535


def _pairs(x):
    return np.asarray(x).reshape(-1, 2).astype(np.int64)


def cfilter_ref(x, head, taps, shift, decim, phase, out_size):
    """-> (out int8 / int16 [nout, 2], clipped): the window of every output against the taps, in int64."""
    x = _pairs(x)
    taps = _pairs(taps)
    nt = len(taps)
    assert int(np.abs(taps).sum()) <= TAP_SUM
    h = np.zeros((nt - 1, 2), np.int64) if head is None else _pairs(head)
    assert len(h) == nt - 1
    nout, _ = span(len(x), decim, phase)
    dtype = np.int8 if out_size == 1 else np.int16
    if nout == 0:
        return np.zeros((0, 2), dtype), 0
    ext = np.concatenate([h, x])                                   # ext[m + nt - 1] = x(m)
    m = phase + decim * np.arange(nout)
    acc = np.zeros((nout, 2), np.int64)
    for k0 in range(0, nt, 64):                                    # in slabs of taps: the index matrix stays small
        k = np.arange(k0, min(k0 + 64, nt))
        w = ext[(m[:, None] - k[None, :]) + nt - 1]                # [nout, slab, 2]
        re, im = taps[k, 0], taps[k, 1]
        acc[:, 0] += w[:, :, 0] @ re - w[:, :, 1] @ im
        acc[:, 1] += w[:, :, 1] @ re + w[:, :, 0] @ im
    assert np.abs(acc).max() < 2 ** 31
    y = acc if shift == 0 else (acc + (1 << (shift - 1))) >> shift  # (>> on int64 floors)
    qmax = 127 if out_size == 1 else 32767
    out = np.clip(y, -qmax, qmax)
    return out.astype(dtype), int(np.count_nonzero(out != y))


def cfilter_scalar(x, head, taps, shift, decim, phase, out_size):
    """The same contract an output and a tap at a time, in Python integers."""
    x = [[int(v) for v in s] for s in np.asarray(x).reshape(-1, 2)]
    taps = [[int(v) for v in t] for t in np.asarray(taps).reshape(-1, 2)]
    nt = len(taps)
    h = None if head is None else [[int(v) for v in s] for s in np.asarray(head).reshape(-1, 2)]
    qmax = 127 if out_size == 1 else 32767
    out, clipped, j = [], 0, 0
    while phase + j * decim < len(x):
        mj = phase + j * decim
        ai = aq = 0
        for k in range(nt):
            m = mj - k
            if m >= 0:
                vi, vq = x[m]
            elif h is not None and m >= -(nt - 1):
                vi, vq = h[nt - 1 + m]
            else:
                vi = vq = 0
            re, im = taps[k]
            ai += re * vi - im * vq
            aq += re * vq + im * vi
        row = []
        for acc in (ai, aq):
            y = acc if shift == 0 else (acc + 2 ** (shift - 1)) // 2 ** shift
            o = min(max(y, -qmax), qmax)
            clipped += o != y
            row.append(o)
        out.append(row)
        j += 1
    return np.array(out, dtype=np.int8 if out_size == 1 else np.int16).reshape(-1, 2), clipped


def cfilter_windows(x_at, nsamp, taps, shift, decim, phase, out_size, outputs):
    """Outputs `outputs` (indices j) of a span too long to filter whole: x_at(lo, hi) returns samples [lo, hi) of the span as [n, 2]
    (0 <= lo <= hi <= nsamp); no head.  -> out [len(outputs), 2]."""
    nt = len(taps)
    rows = []
    for j in outputs:
        mj = phase + int(j) * decim
        assert 0 <= mj < nsamp
        lo = max(mj - (nt - 1), 0)
        o, _ = cfilter_ref(_pairs(x_at(lo, mj + 1)), None, taps, shift, 1, 0, out_size)
        rows.append(o[-1])
    return np.array(rows).reshape(-1, 2)


def notch_find(power, fs, ratio, max_lines):
    """gpsiq_notch_find in Python integers and fractions -> (f_hz list, excess_db list, nlines), or None where the call refuses (a
    floor of 0).  `ratio` is taken as the exact value of the double (the library compares in long double: the two agree wherever
    ratio * floor is exact there, which holds for the ratios and powers the tests use)."""
    p = [int(v) for v in power]
    n = len(p)
    floor = sorted(p)[n // 2 - 1]
    if floor == 0:
        return None
    limit = Fraction(ratio) * floor
    over = [v > limit for v in p]
    start = over.index(False)
    lines, i = [], 1
    while i <= n:
        k0 = (start + i) % n
        if not over[k0]:
            i += 1
            continue
        length = 0
        while over[(k0 + length) % n]:
            length += 1
        cells = [p[(k0 + d) % n] for d in range(length)]
        pos = Fraction(sum(v * d for d, v in enumerate(cells)), sum(cells)) + (k0 if k0 < n // 2 else k0 - n)
        if pos >= n // 2:
            pos -= n
        lines.append((max(cells), k0, float(pos * Fraction(fs) / n)))
        i += length
    lines.sort(key=lambda t: (-t[0], t[1]))
    keep = lines[:max_lines]
    return [t[2] for t in keep], [10.0 * math.log10(Fraction(t[0], floor)) for t in keep], len(lines)


def response(taps, shift, freqs, fs):
    """H(f) of integer complex taps over 2^shift at the frequencies `freqs`."""
    t = _pairs(taps)
    h = (t[:, 0] + 1j * t[:, 1]) / float(1 << shift)
    n = np.arange(len(h))
    return np.exp(-2j * np.pi * np.outer(np.asarray(freqs, dtype=np.float64) / fs, n)) @ h


def prototype(ntaps, cutoff_over_fs):
    """g of gpsiq_notch_design: gpsiq_filter_design's Hamming-windowed sinc at cutoff `cutoff_over_fs` * fs, unrounded, sum 1."""
    k = np.arange(ntaps)
    mid = (ntaps - 1) / 2
    g = 2 * cutoff_over_fs * np.sinc(2 * cutoff_over_fs * (k - mid)) * (0.54 - 0.46 * np.cos(2 * np.pi * k / (ntaps - 1)))
    return g / g.sum()


# ---- the notch chain's stream (tests/test_cfilter_ref.py on the restatements, tests/test_gpu_notch_signal.py on the device) ----------
NOTCH_FS, NOTCH_NSAMP, NOTCH_NFFT, NOTCH_HOP = 2.6e6, 8192, 256, 128
NOTCH_SIGMA, NOTCH_AMP, NOTCH_SEED, NOTCH_RATIO = 200.0, 8000.0, 20261, 8.0
NOTCH_NTAPS, NOTCH_WIDTH_BINS, NOTCH_SHIFT = 129, 4, 12
NOTCH_CASES = {"one": (37,), "two": (37, -90)}


def notch_stream(bins):
    """int16 [8192, 2]: seeded Gaussian noise, sigma 200 per component, plus a tone of amplitude 8000 on each of `bins` of 256"""
    rng = np.random.default_rng(NOTCH_SEED)
    z = rng.normal(0.0, NOTCH_SIGMA, size=(NOTCH_NSAMP, 2))
    n = np.arange(NOTCH_NSAMP)
    for b in bins:
        ph = 2 * np.pi * b * n / NOTCH_NFFT
        z[:, 0] += NOTCH_AMP * np.cos(ph)
        z[:, 1] += NOTCH_AMP * np.sin(ph)
    x = np.rint(z)
    assert np.abs(x).max() <= 32767
    return x.astype(np.int16)


def bin_hz(b):
    return b * NOTCH_FS / NOTCH_NFFT
