"""The contract of gpsiq_agc (include/gpsiq_rows.h, "AGC") restated in numpy, with Python integers for the gain rule: blanker, windowed
power, ring, multipliers, output, counts and the state a span leaves.  TEST INFRASTRUCTURE: the device call, the batch call and the
host arithmetic of the library are each held to this file, never the other way round."""
import collections
import math

import numpy as np

Cfg = collections.namedtuple("Cfg", "window navg target_q8 mult0 mult_min mult_max blank_thresh blank_hold qmax")
# ring: list of (sum, count) of the last complete windows, oldest first; psum / pcnt / fill: the window in progress; hold
State = collections.namedtuple("State", "ring psum pcnt fill hold")
FRESH = State((), 0, 0, 0, 0)


def cfg(window=1024, navg=16, target_q8=256, mult0=65536, mult_min=1, mult_max=(1 << 24) - 1, blank_thresh=0, blank_hold=0, qmax=127):
    return Cfg(window, navg, target_q8, mult0, mult_min, mult_max, blank_thresh, blank_hold, qmax)


def mult(c, sumsq, count):
    """the gain rule"""
    S, n = int(sumsq), int(count)
    if n == 0:
        return c.mult0
    m = ((S // n) << 16) + (((S % n) << 16) // n)
    assert m == (S << 16) // n
    r = max(math.isqrt(m), 1)
    return min(max((c.target_q8 << 16) // r, c.mult_min), c.mult_max)


def span(nsamp, window, fill=0):
    """(windows touched, the fill the span leaves)"""
    return (-(-(fill + nsamp) // window) if nsamp else 0), (fill + nsamp) % window


def full_range(rng, n, sample_size):
    """[n, 2] random elements over the whole range of the format, both extremes present"""
    lo, hi, dt = (-128, 127, np.int8) if sample_size == 1 else (-32768, 32767, np.int16)
    x = rng.integers(lo, hi + 1, size=(n, 2)).astype(dt)
    if n >= 2:
        x[0, 0], x[-1, 1] = lo, hi
    return x


def blank_flags(x, c, hold_in):
    """(blank [n] bool, the hold the span leaves)"""
    n = len(x)
    idx = np.arange(n, dtype=np.int64)
    a = np.abs(x.astype(np.int64))
    exceed = (a > c.blank_thresh).any(axis=1) if c.blank_thresh > 0 else np.zeros(n, bool)
    last = np.maximum.accumulate(np.where(exceed, idx, -(1 << 40))) if n else idx
    blank = (idx < hold_in) | (last >= idx - c.blank_hold)
    hold = max(0, hold_in - n)
    if exceed.any():
        hold = max(hold, c.blank_hold - (n - 1 - int(np.flatnonzero(exceed)[-1])))
    return blank, hold


def agc_ref(x, c, state=FRESH, out_sample_size=1):
    """x [n, 2] int8 / int16 -> (out [n, 2] of out_sample_size, clipped, blanked, mults [nwin] list, the state the span leaves)"""
    x = np.asarray(x)
    n, W, M = len(x), c.window, c.navg
    assert x.ndim == 2 and x.shape[1] == 2 and len(state.ring) <= M and state.fill < W and state.pcnt <= 2 * state.fill and state.hold <= c.blank_hold
    odt = np.int8 if out_sample_size == 1 else np.int16
    if n == 0:
        return np.zeros((0, 2), odt), 0, 0, [], state
    blank, hold = blank_flags(x, c, state.hold)
    xi = x.astype(np.int64)
    power = np.where(blank, 0, (xi * xi).sum(axis=1))
    ring, psum, pcnt, fill = list(state.ring), state.psum, state.pcnt, state.fill
    gains = np.zeros(n, np.int64)
    mults = []
    at = 0
    while at < n:
        take = min(W - fill, n - at)
        g = mult(c, sum(s for s, _ in ring), sum(k for _, k in ring))          # fixed at the window's start: the ring as it is now
        mults.append(g)
        gains[at:at + take] = g
        psum += int(power[at:at + take].sum())
        pcnt += 2 * int((~blank[at:at + take]).sum())
        fill += take
        at += take
        if fill == W:
            ring = (ring + [(psum, pcnt)])[-M:]
            psum = pcnt = fill = 0
    y = (xi * gains[:, None] + 32768) >> 16
    out = np.clip(y, -c.qmax, c.qmax)
    clipped = int(((out != y) & ~blank[:, None]).sum())
    out[blank] = 0
    return out.astype(odt), clipped, int(blank.sum()), mults, State(tuple(ring), psum, pcnt, fill, hold)


def in_pieces(x, c, cuts, state=FRESH, out_sample_size=1):
    """the same span cut at `cuts`, each piece from the state the piece before left: what one call must equal.  The multiplier of a
    window continued across a cut is listed once"""
    outs, clipped, blanked, mults = [], 0, 0, []
    edges = [0] + list(cuts) + [len(x)]
    for lo, hi in zip(edges, edges[1:]):
        continued = state.fill > 0 and hi > lo
        o, cl, bl, mu, state = agc_ref(x[lo:hi], c, state, out_sample_size)
        if continued and mults:
            assert mu[0] == mults[-1], "a window continued across a call repeats its multiplier"
            mu = mu[1:]
        outs.append(o)
        clipped, blanked, mults = clipped + cl, blanked + bl, mults + mu
    return np.concatenate(outs), clipped, blanked, mults, state


# ---- the library's structures ------------------------------------------------------------------------------------------------------
def to_lib_cfg(c):
    import gpsiq
    return gpsiq.AgcCfg(*c)


def to_lib_state(s):
    import gpsiq
    st = gpsiq.AgcState()
    for r, (a, k) in enumerate(s.ring):
        st.wsum[r], st.wcnt[r] = a, k
    st.psum, st.pcnt, st.fill, st.nring, st.hold = s.psum, s.pcnt, s.fill, len(s.ring), s.hold
    return st


def from_lib_state(st):
    """-> State; entries of the ring beyond nring must be zeros"""
    assert all(st.wsum[r] == 0 and st.wcnt[r] == 0 for r in range(int(st.nring), 64)), "ring entries beyond nring are not zero"
    return State(tuple((int(st.wsum[r]), int(st.wcnt[r])) for r in range(int(st.nring))), int(st.psum), int(st.pcnt), int(st.fill), int(st.hold))
