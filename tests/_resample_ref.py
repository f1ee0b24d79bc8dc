"""gpsiq_resample restated in numpy from its contract (include/gpsiq_rows.h, "Resample"), and a second, scalar statement of the same
contract beside it.  TEST INFRASTRUCTURE: neither reads a line of the library.

Streams are integer arrays [n, 2] (I, Q) or flat interleaved [2 n]; `head` is the ntaps - 1 samples before the span or None (zeros);
`taps` is [2**L + 1, ntaps]; positions and steps are Python integers in units of 2**-32 input sample."""
import numpy as np

ONE = 1 << 32


def span(nsamp, pos0, step):
    """(nout, next_pos) of the contract, in Python integers."""
    end = nsamp * ONE
    nout = 0 if pos0 >= end else -((pos0 - end) // step)           # ceil((end - pos0) / step)
    return nout, pos0 + nout * step - end


def _pairs(x):
    return np.asarray(x).reshape(-1, 2).astype(np.int64)


def _table(taps, L):
    taps = np.asarray(taps, dtype=np.int64)
    assert taps.ndim == 2 and taps.shape[0] == (1 << L) + 1, taps.shape
    return taps


def _core(ext, off, j, taps, L, shift, interp, step, pos0, out_size):
    """outputs j (an int array) where x(m) = ext[m + off] for every m they need -> (out [len(j), 2], clipped)"""
    nt = taps.shape[1]
    p = np.uint64(pos0) + np.asarray(j, dtype=np.uint64) * np.uint64(step)            # below nsamp * 2^32 < 2^63: no wrap
    m = (p >> np.uint64(32)).astype(np.int64)
    f = (p & np.uint64(0xFFFFFFFF)).astype(np.int64)
    q = f >> (32 - L)                                               # (int64: a shift by 32 at L == 0 gives 0)
    mu = (f >> (24 - L)) & 255 if interp else np.zeros_like(f)
    k = np.arange(nt)
    win = ext[(m[:, None] - k[None, :]) + off]                      # [j, k, c]
    a0 = np.einsum("jk,jkc->jc", taps[q], win)
    if interp:
        a1 = np.einsum("jk,jkc->jc", taps[q + 1], win)
        y = ((256 - mu)[:, None] * a0 + mu[:, None] * a1 + (1 << (shift + 7))) >> (shift + 8)
    else:
        y = a0 if shift == 0 else (a0 + (1 << (shift - 1))) >> shift                  # (>> on int64 floors)
    qmax = 127 if out_size == 1 else 32767
    out = np.clip(y, -qmax, qmax)
    return out.astype(np.int8 if out_size == 1 else np.int16), int(np.count_nonzero(out != y))


def resample_ref(x, head, taps, L, shift, interp, step, pos0, out_size, j_lo=0, j_hi=None):
    """-> (out int8 / int16 [j_hi - j_lo, 2], clipped among them, nout, next_pos): outputs [j_lo, j_hi) of the span, all by default"""
    x = _pairs(x)
    taps = _table(taps, L)
    nt = taps.shape[1]
    h = np.zeros((nt - 1, 2), np.int64) if head is None else _pairs(head)
    assert len(h) == nt - 1
    nout, nxt = span(len(x), pos0, step)
    j_hi = nout if j_hi is None else j_hi
    assert 0 <= j_lo <= j_hi <= nout
    if j_hi == j_lo:
        return np.zeros((0, 2), np.int8 if out_size == 1 else np.int16), 0, nout, nxt
    ext = np.concatenate([h, x])                                   # ext[m + nt - 1] = x(m)
    outs, clipped = [], 0
    for lo in range(j_lo, j_hi, 1 << 16):                          # in slabs of outputs: the index matrix stays small
        o, c = _core(ext, nt - 1, np.arange(lo, min(lo + (1 << 16), j_hi)), taps, L, shift, interp, step, pos0, out_size)
        outs.append(o)
        clipped += c
    return np.concatenate(outs), clipped, nout, nxt


def resample_scalar(x, head, taps, L, shift, interp, step, pos0, out_size):
    """The same contract an output and a tap at a time, in Python integers -> (out, clipped, nout, next_pos)."""
    x = [[int(v) for v in s] for s in np.asarray(x).reshape(-1, 2)]
    taps = [[int(t) for t in row] for row in np.asarray(taps)]
    nt = len(taps[0])
    h = None if head is None else [[int(v) for v in s] for s in np.asarray(head).reshape(-1, 2)]
    qmax = 127 if out_size == 1 else 32767
    out, clipped, j = [], 0, 0
    while (pos0 + j * step) >> 32 < len(x):
        p = pos0 + j * step
        mj, f = p >> 32, p & 0xFFFFFFFF
        q = f >> (32 - L) if L else 0
        mu = (f >> (24 - L)) & 255 if interp else 0
        row = []
        for c in (0, 1):
            a = [0, 0]
            for k in range(nt):
                m = mj - k
                v = x[m][c] if m >= 0 else h[nt - 1 + m][c] if h is not None and m >= -(nt - 1) else 0
                a[0] += taps[q][k] * v
                if interp:
                    a[1] += taps[q + 1][k] * v
            assert abs(a[0]) < 2 ** 31 and abs(a[1]) < 2 ** 31
            if interp:
                y = ((256 - mu) * a[0] + mu * a[1] + 2 ** (shift + 7)) // 2 ** (shift + 8)
            else:
                y = a[0] if shift == 0 else (a[0] + 2 ** (shift - 1)) // 2 ** shift
            o = min(max(y, -qmax), qmax)
            clipped += o != y
            row.append(o)
        out.append(row)
        j += 1
    nxt = pos0 + j * step - len(x) * ONE
    return np.array(out, dtype=np.int8 if out_size == 1 else np.int16).reshape(-1, 2), clipped, j, nxt


def resample_window(x_at, nsamp, taps, L, shift, interp, step, pos0, out_size, j_lo, j_hi):
    """Outputs [j_lo, j_hi) of a span too long to resample whole: x_at(lo, hi) returns samples [lo, hi) of the span as [n, 2]
    (0 <= lo <= hi <= nsamp); no head.  -> (out [j_hi - j_lo, 2], clipped among them)"""
    taps = _table(taps, L)
    nt = taps.shape[1]
    m_lo, m_hi = (pos0 + j_lo * step) >> 32, (pos0 + (j_hi - 1) * step) >> 32
    assert j_lo < j_hi and m_hi < nsamp
    lo = max(m_lo - (nt - 1), 0)
    ext = np.concatenate([np.zeros((nt - 1, 2), np.int64), _pairs(x_at(lo, m_hi + 1))])          # ext[m - lo + nt - 1] = x(m), zeros before sample 0
    return _core(ext, nt - 1 - lo, np.arange(j_lo, j_hi), taps, L, shift, interp, step, pos0, out_size)


def full_range(rng, n, size):
    """n samples of full-range elements of the format, the most negative value included."""
    lo, hi = (-128, 127) if size == 1 else (-32768, 32767)
    x = rng.integers(lo, hi + 1, size=(n, 2)).astype(np.int8 if size == 1 else np.int16)
    if n:
        x[rng.integers(0, n), rng.integers(0, 2)] = lo
    return x


def random_table(rng, L, ntaps, total=None):
    """int16 rows of both signs [2**L + 1, ntaps]; total: every row's sum of magnitudes exactly (at most 65535; three taps or more)"""
    rows = (1 << L) + 1
    lim = max(60000 // ntaps // 2, 1)
    t = rng.integers(-lim, lim + 1, size=(rows, ntaps)).astype(np.int64)
    if total is not None:
        for r in range(rows):
            for k in range(ntaps):
                add = min(total - int(np.abs(t[r]).sum()), 32767 - abs(int(t[r, k])))
                t[r, k] += add * (1 if t[r, k] >= 0 else -1)
            assert int(np.abs(t[r]).sum()) == total
    return t.astype(np.int16)


def alternating_table(L, ntaps):
    """rows whose absolute sum is 65535 with alternating signs, each row starting on the other sign than the one before"""
    rows = (1 << L) + 1
    base = np.full(ntaps, 65535 // ntaps, np.int64)
    base[: 65535 - int(base.sum())] += 1
    assert int(base.sum()) == 65535 and int(base.max()) <= 32767
    sign = np.where(np.arange(ntaps) % 2 == 0, 1, -1)
    return np.stack([base * sign * (1 if r % 2 == 0 else -1) for r in range(rows)]).astype(np.int16)
