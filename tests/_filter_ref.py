"""gpsiq_filter restated in numpy from its contract (include/gpsiq_rows.h, "Filter"), and a second, scalar statement of the same
contract beside it.  TEST INFRASTRUCTURE: neither reads a line of the library.

Streams are integer arrays [n, 2] (I, Q) or flat interleaved [2 n]; `head` is the ntaps - 1 samples before the span or None (zeros)."""
import numpy as np


def span(nsamp, decim, phase):
    """(nout, next_phase) of the contract."""
    nout = 0 if phase >= nsamp else (nsamp - phase + decim - 1) // decim
    return nout, phase + nout * decim - nsamp


def _pairs(x):
    return np.asarray(x).reshape(-1, 2).astype(np.int64)


def filter_ref(x, head, taps, shift, decim, phase, out_size):
    """-> (out int8 / int16 [nout, 2], clipped): a matrix of the window of every output against the taps, in int64."""
    x = _pairs(x)
    taps = np.asarray(taps, dtype=np.int64).ravel()
    nt = len(taps)
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
        acc += np.einsum("k,jkc->jc", taps[k], ext[(m[:, None] - k[None, :]) + nt - 1])
    y = acc if shift == 0 else (acc + (1 << (shift - 1))) >> shift  # (>> on int64 floors)
    qmax = 127 if out_size == 1 else 32767
    out = np.clip(y, -qmax, qmax)
    return out.astype(dtype), int(np.count_nonzero(out != y))


def filter_scalar(x, head, taps, shift, decim, phase, out_size):
    """The same contract an output and a tap at a time, in Python integers."""
    x = [[int(v) for v in s] for s in np.asarray(x).reshape(-1, 2)]
    taps = [int(t) for t in np.asarray(taps).ravel()]
    nt = len(taps)
    h = None if head is None else [[int(v) for v in s] for s in np.asarray(head).reshape(-1, 2)]
    qmax = 127 if out_size == 1 else 32767
    out, clipped, j = [], 0, 0
    while phase + j * decim < len(x):
        mj = phase + j * decim
        row = []
        for c in (0, 1):
            acc = 0
            for k in range(nt):
                m = mj - k
                if m >= 0:
                    v = x[m][c]
                elif h is not None and m >= -(nt - 1):
                    v = h[nt - 1 + m][c]
                else:
                    v = 0
                acc += taps[k] * v
            y = acc if shift == 0 else (acc + 2 ** (shift - 1)) // 2 ** shift
            o = min(max(y, -qmax), qmax)
            clipped += o != y
            row.append(o)
        out.append(row)
        j += 1
    return np.array(out, dtype=np.int8 if out_size == 1 else np.int16).reshape(-1, 2), clipped


def filter_windows(x_at, nsamp, taps, shift, decim, phase, out_size, outputs):
    """Outputs `outputs` (indices j) of a span too long to filter whole: x_at(lo, hi) returns samples [lo, hi) of the span as [n, 2]
    (0 <= lo <= hi <= nsamp); no head.  -> out [len(outputs), 2]."""
    nt = len(taps)
    rows = []
    for j in outputs:
        mj = phase + int(j) * decim
        assert 0 <= mj < nsamp
        lo = max(mj - (nt - 1), 0)
        w = _pairs(x_at(lo, mj + 1))                                # every tap's sample, or from sample 0 on with zeros before it
        o, _ = filter_ref(w, None, taps, shift, 1, 0, out_size)
        rows.append(o[-1])
    return np.array(rows).reshape(-1, 2)


def full_range(rng, n, size):
    """n samples of full-range elements of the format, the most negative value included."""
    lo, hi = (-128, 127) if size == 1 else (-32768, 32767)
    x = rng.integers(lo, hi + 1, size=(n, 2)).astype(np.int8 if size == 1 else np.int16)
    if n:
        x[rng.integers(0, n), rng.integers(0, 2)] = lo
    return x
