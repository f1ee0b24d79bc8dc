"""gpsiq_stap_cov and gpsiq_stap_combine restated from their contract (include/gpsiq_rows.h, "Space-time array"): numpy in int64
(exact: a term is at most 2^31 and there are fewer than 2^31 of them), a scalar statement in Python integers beside it, and the seeded
integer scene of a broadband jammer with one echo that the stage exists for.  TEST INFRASTRUCTURE: nothing here reads a line of the
library, and nothing goes through tests/_array_ref.py or tests/_cfilter_ref.py -- the identities with those are tests.

Streams are integer arrays [n, 2] (I, Q); `xs` is a sequence of nelem of them, equally long; `heads` is None or a sequence of nelem
entries, each None (zeros) or the ntaps - 1 samples [ntaps - 1, 2] before the span; weights are [nelem, ntaps, 2] (re, im).  Row
k = e * ntaps + t is z_k(n) = x_e(n - t)."""
import numpy as np

WEIGHT_SUM = 65535
MAX_ELEM, MAX_TAPS, MAX_ROWS = 8, 8, 32


def _pairs(x):
    return np.asarray(x).reshape(-1, 2).astype(np.int64)


def extended(x, head, ntaps):
    """int64 [ntaps - 1 + n, 2]: x with the samples before the span in front of it: x_e(m) at row m + ntaps - 1"""
    x = _pairs(x)
    h = np.zeros((ntaps - 1, 2), np.int64) if head is None else _pairs(head)
    assert len(h) == ntaps - 1
    return np.concatenate([h, x])


def rows(xs, heads, ntaps):
    """the K rows as int64 arrays [n, 2], k = e * ntaps + t"""
    assert 1 <= len(xs) <= MAX_ELEM and 1 <= ntaps <= MAX_TAPS and len(xs) * ntaps <= MAX_ROWS
    heads = [None] * len(xs) if heads is None else list(heads)
    assert len(heads) == len(xs)
    out = []
    for x, h in zip(xs, heads):
        ext = extended(x, h, ntaps)
        n = len(ext) - (ntaps - 1)
        for t in range(ntaps):
            out.append(ext[ntaps - 1 - t:ntaps - 1 - t + n])
    return out


def cov_ref(xs, heads, ntaps):
    """-> int64 [K, K, 2]: R[k][l] = sum z_k conj(z_l), re = sum Ik Il + Qk Ql, im = sum Qk Il - Ik Ql"""
    z = rows(xs, heads, ntaps)
    k = len(z)
    if not len(z[0]):
        return np.zeros((k, k, 2), np.int64)
    i = np.stack([r[:, 0] for r in z])
    q = np.stack([r[:, 1] for r in z])
    out = np.zeros((k, k, 2), np.int64)
    out[:, :, 0] = i @ i.T + q @ q.T
    out[:, :, 1] = q @ i.T - i @ q.T
    return out


def x_at(x, head, ntaps, m):
    """x_e(m) of the contract in Python integers, -(ntaps - 1) <= m < n"""
    if m >= 0:
        return int(x[m][0]), int(x[m][1])
    if head is None:
        return 0, 0
    return int(head[ntaps - 1 + m][0]), int(head[ntaps - 1 + m][1])


def cov_scalar(xs, heads, ntaps):
    """The same contract a sample and an entry at a time, in Python integers -> nested lists [K][K][2]."""
    xs = [np.asarray(x).reshape(-1, 2) for x in xs]
    heads = [None] * len(xs) if heads is None else [None if h is None else np.asarray(h).reshape(-1, 2) for h in heads]
    kk = len(xs) * ntaps
    out = [[[0, 0] for _ in range(kk)] for _ in range(kk)]
    for k in range(kk):
        for l in range(kk):
            for n in range(len(xs[0])):
                ia, qa = x_at(xs[k // ntaps], heads[k // ntaps], ntaps, n - k % ntaps)
                ib, qb = x_at(xs[l // ntaps], heads[l // ntaps], ntaps, n - l % ntaps)
                out[k][l][0] += ia * ib + qa * qb
                out[k][l][1] += qa * ib - ia * qb
    return out


def finish(acc, shift, out_size):
    """gpsiq_cfilter's finish on an int64 array -> (clamped int64 array, elements the clamp changed)"""
    assert np.abs(acc).max(initial=0) < 2 ** 31
    y = acc if shift == 0 else (acc + (1 << (shift - 1))) >> shift     # (>> on int64 floors)
    qmax = 127 if out_size == 1 else 32767
    out = np.clip(y, -qmax, qmax)
    return out, int(np.count_nonzero(out != y))


def combine_ref(xs, heads, w, shift, out_size):
    """-> (out int8 / int16 [n, 2], clipped): y(n) = sum over e, t of w[e][t] x_e(n - t)"""
    w = np.asarray(w).astype(np.int64)
    assert w.ndim == 3 and w.shape[0] == len(xs) and w.shape[2] == 2 and int(np.abs(w).sum()) <= WEIGHT_SUM
    ntaps = w.shape[1]
    z = rows(xs, heads, ntaps)
    acc = np.zeros((len(z[0]), 2), np.int64)
    for r, (re, im) in zip(z, w.reshape(-1, 2)):
        acc[:, 0] += re * r[:, 0] - im * r[:, 1]
        acc[:, 1] += re * r[:, 1] + im * r[:, 0]
    out, clipped = finish(acc, shift, out_size)
    return out.astype(np.int8 if out_size == 1 else np.int16), clipped


def combine_scalar(xs, heads, w, shift, out_size):
    """The same contract a sample at a time, in Python integers."""
    xs = [np.asarray(x).reshape(-1, 2) for x in xs]
    heads = [None] * len(xs) if heads is None else [None if h is None else np.asarray(h).reshape(-1, 2) for h in heads]
    w = np.asarray(w)
    ntaps = w.shape[1]
    qmax = 127 if out_size == 1 else 32767
    out, clipped = [], 0
    for n in range(len(xs[0])):
        ai = aq = 0
        for e in range(len(xs)):
            for t in range(ntaps):
                re, im = int(w[e][t][0]), int(w[e][t][1])
                i, q = x_at(xs[e], heads[e], ntaps, n - t)
                ai += re * i - im * q
                aq += re * q + im * i
        row = []
        for acc in (ai, aq):
            y = acc if shift == 0 else (acc + 2 ** (shift - 1)) // 2 ** shift
            o = min(max(y, -qmax), qmax)
            clipped += o != y
            row.append(o)
        out.append(row)
    return np.array(out, dtype=np.int8 if out_size == 1 else np.int16).reshape(-1, 2), clipped


def quadratic_form(w, cov):
    """sum over k, l of w_k conj(w_l) R[k][l] in Python integers -> (re, im), w [nelem, ntaps, 2] or [K, 2]"""
    w = [[int(v) for v in t] for t in np.asarray(w).reshape(-1, 2)]
    re = im = 0
    for a, (ar, ai) in enumerate(w):
        for b, (br, bi) in enumerate(w):
            pr, pi = ar * br + ai * bi, ai * br - ar * bi              # w_a conj(w_b)
            rr, ri = int(cov[a][b][0]), int(cov[a][b][1])
            re += pr * rr - pi * ri
            im += pr * ri + pi * rr
    return re, im


def heads_of(pool, at, ntaps):
    """the ntaps - 1 samples before sample `at` of every stream of pool (at >= ntaps - 1)"""
    return [x[at - (ntaps - 1):at] for x in pool]


def streams(rng, nelem, nsamp, in_size, kind="random"):
    """nelem test streams [nsamp, 2]: uniform over the format's whole range, or its extremes at random"""
    dtype = np.int8 if in_size == 1 else np.int16
    lo, hi = (-128, 127) if in_size == 1 else (-32768, 32767)
    if kind == "extremes":
        return [np.where(rng.integers(0, 2, size=(nsamp, 2)) == 1, hi, lo).astype(dtype) for _ in range(nelem)]
    return [rng.integers(lo, hi + 1, size=(nsamp, 2)).astype(dtype) for _ in range(nelem)]


# ---- the scene: a broadband jammer that arrives twice ------------------------------------------------------------------------------
# Two elements.  The jammer j(n), white complex Gaussian of power J = 10^(jn_db / 10) against noise of power 1, reaches element e
# directly with the Gaussian-integer gain DIRECT[e] / SCALE and again d samples later with ECHO[e] / SCALE; the streams are scaled by
# SCALE and rounded, as a receiver's converter would.  The gains are chosen so that the two arrivals' spatial signatures differ by
# 129 degrees more than a common phase: the best two-element combination with w_0 = 1 then leaves
#   |a_0|^2 + |b_0|^2 - |a_0 conj(a_1) + b_0 conj(b_1)|^2 / (|a_1|^2 + |b_1|^2) = 1.07 |a_0|^2   of the jammer, +0.3 dB:
# space alone does nothing, which is what the stage's issue measured with amplitude 0.7 for the echo.
SCALE = 16
DIRECT = (16 + 0j, 0 + 16j)
ECHO = (11 + 0j, 9 - 7j)


def echo_scene(seed, nsamp, d, jn_db, nelem=2):
    """-> (xs: nelem int16 streams [nsamp, 2], jammer power at element 0 by its direct path in stream units squared, noise power in the
    same units).  The echo's first d samples see the jammer's own past, so the scene has no start-up transient."""
    assert nelem == 2 and 1 <= d <= 7
    rng = np.random.default_rng(seed)
    amp = np.sqrt(10.0 ** (jn_db / 10.0) / 2.0)
    j = amp * (rng.standard_normal(nsamp + d) + 1j * rng.standard_normal(nsamp + d))
    xs = []
    for e in range(nelem):
        noise = np.sqrt(0.5) * (rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp))
        x = DIRECT[e] * j[d:] + ECHO[e] * j[:nsamp] + SCALE * noise
        s = np.stack([np.rint(x.real), np.rint(x.imag)], axis=1)
        assert np.abs(s).max() <= 32767
        xs.append(s.astype(np.int16))
    return xs, abs(DIRECT[0]) ** 2 * 10.0 ** (jn_db / 10.0), float(SCALE * SCALE)


def power(y):
    """mean |y|^2 of a stream [n, 2]"""
    y = _pairs(y).astype(np.float64)
    return float((y * y).sum() / len(y))
