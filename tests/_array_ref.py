"""gpsiq_array_cov and gpsiq_array_combine restated from their contract (include/gpsiq_rows.h, "Array"): numpy in int64 (exact: a term
is at most 2^31 and there are fewer than 2^31 of them), a scalar statement in Python integers beside it.  TEST INFRASTRUCTURE: nothing
here reads a line of the library.

Streams are integer arrays [n, 2] (I, Q) or flat interleaved [2 n]; `xs` is a sequence of nelem of them, equally long; weights are
[nelem, 2] (re, im)."""
import numpy as np

WEIGHT_SUM = 65535
MAX_ELEM = 8
SQUARE = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.5, 0.5, 0.0]])    # four elements, half a wavelength apart


def _pairs(x):
    return np.asarray(x).reshape(-1, 2).astype(np.int64)


def cov_ref(xs, chunk=1 << 20):
    """-> int64 [E, E, 2]: R[a][b] = sum x_a conj(x_b), re = sum Ia Ib + Qa Qb, im = sum Qa Ib - Ia Qb; in chunks, so that a long span
    needs no int64 copy of itself"""
    e = len(xs)
    n = len(np.asarray(xs[0]).reshape(-1, 2))
    out = np.zeros((e, e, 2), np.int64)
    for lo in range(0, n, chunk):
        part = [_pairs(np.asarray(x).reshape(-1, 2)[lo:lo + chunk]) for x in xs]
        i = np.stack([p[:, 0] for p in part])                          # [E, m]
        q = np.stack([p[:, 1] for p in part])
        out[:, :, 0] += i @ i.T + q @ q.T
        out[:, :, 1] += q @ i.T - i @ q.T
    return out


def cov_scalar(xs):
    """The same contract a sample and an entry at a time, in Python integers -> nested lists [E][E][2]."""
    xs = [[[int(v) for v in s] for s in np.asarray(x).reshape(-1, 2)] for x in xs]
    e = len(xs)
    out = [[[0, 0] for _ in range(e)] for _ in range(e)]
    for a in range(e):
        for b in range(e):
            for (ia, qa), (ib, qb) in zip(xs[a], xs[b]):
                out[a][b][0] += ia * ib + qa * qb
                out[a][b][1] += qa * ib - ia * qb
    return out


def finish(acc, shift, out_size):
    """gpsiq_cfilter's finish on an int64 array -> (clamped int64 array, elements the clamp changed)"""
    assert np.abs(acc).max(initial=0) < 2 ** 31
    y = acc if shift == 0 else (acc + (1 << (shift - 1))) >> shift     # (>> on int64 floors)
    qmax = 127 if out_size == 1 else 32767
    out = np.clip(y, -qmax, qmax)
    return out, int(np.count_nonzero(out != y))


def combine_ref(xs, w, shift, out_size):
    """-> (out int8 / int16 [n, 2], clipped)"""
    w = _pairs(w)
    assert len(w) == len(xs) and int(np.abs(w).sum()) <= WEIGHT_SUM
    n = len(np.asarray(xs[0]).reshape(-1, 2))
    acc = np.zeros((n, 2), np.int64)
    for x, (re, im) in zip(xs, w):
        x = _pairs(x)
        acc[:, 0] += re * x[:, 0] - im * x[:, 1]
        acc[:, 1] += re * x[:, 1] + im * x[:, 0]
    out, clipped = finish(acc, shift, out_size)
    return out.astype(np.int8 if out_size == 1 else np.int16), clipped


def combine_scalar(xs, w, shift, out_size):
    """The same contract a sample at a time, in Python integers."""
    xs = [[[int(v) for v in s] for s in np.asarray(x).reshape(-1, 2)] for x in xs]
    w = [[int(v) for v in t] for t in np.asarray(w).reshape(-1, 2)]
    qmax = 127 if out_size == 1 else 32767
    out, clipped = [], 0
    for n in range(len(xs[0])):
        ai = sum(re * x[n][0] - im * x[n][1] for x, (re, im) in zip(xs, w))
        aq = sum(re * x[n][1] + im * x[n][0] for x, (re, im) in zip(xs, w))
        row = []
        for acc in (ai, aq):
            y = acc if shift == 0 else (acc + 2 ** (shift - 1)) // 2 ** shift
            o = min(max(y, -qmax), qmax)
            clipped += o != y
            row.append(o)
        out.append(row)
    return np.array(out, dtype=np.int8 if out_size == 1 else np.int16).reshape(-1, 2), clipped


def quadratic_form(w, cov):
    """sum over a, b of w_a conj(w_b) R[a][b] in Python integers -> (re, im): the power of the combined stream before any shift"""
    w = [[int(v) for v in t] for t in np.asarray(w).reshape(-1, 2)]
    re = im = 0
    for a, (ar, ai) in enumerate(w):
        for b, (br, bi) in enumerate(w):
            pr, pi = ar * br + ai * bi, ai * br - ar * bi              # w_a conj(w_b)
            rr, ri = int(cov[a][b][0]), int(cov[a][b][1])
            re += pr * rr - pi * ri
            im += pr * ri + pi * rr
    return re, im


def steer_ref(pos, az, el):
    u = np.array([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)])
    return np.mod(np.asarray(pos, dtype=np.float64) @ u, 1.0)


def model_cov(nelem, sigma2, jammers, nsamp, scale=1.0):
    """int64 [E, E, 2] of nsamp * scale * (sigma2 I + sum J a a^H), jammers a list of (J, phases in cycles), rounded to integers and
    made exactly Hermitian; -> (cov, the real matrix Rn = cov / nsamp as complex128)"""
    r = sigma2 * np.eye(nelem, dtype=np.complex128)
    for power, cycles in jammers:
        a = np.exp(2j * np.pi * np.asarray(cycles, dtype=np.float64))
        r += power * np.outer(a, a.conj())
    m = np.rint(r.real * nsamp * scale).astype(np.int64), np.rint(r.imag * nsamp * scale).astype(np.int64)
    cov = np.zeros((nelem, nelem, 2), np.int64)
    for a in range(nelem):
        for b in range(a + 1):
            cov[a, b] = (m[0][a, b], 0 if a == b else m[1][a, b])
            cov[b, a] = (m[0][a, b], 0 if a == b else -m[1][a, b])
    return cov, (cov[:, :, 0] + 1j * cov[:, :, 1]) / float(nsamp)


def streams(rng, nelem, nsamp, in_size, kind="random"):
    """nelem test streams [nsamp, 2]: uniform over the format's whole range, or its extremes at random"""
    dtype = np.int8 if in_size == 1 else np.int16
    lo, hi = (-128, 127) if in_size == 1 else (-32768, 32767)
    if kind == "extremes":
        return [np.where(rng.integers(0, 2, size=(nsamp, 2)) == 1, hi, lo).astype(dtype) for _ in range(nelem)]
    return [rng.integers(lo, hi + 1, size=(nsamp, 2)).astype(dtype) for _ in range(nelem)]
