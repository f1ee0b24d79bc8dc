"""The mix stage restated: include/gpsiq_rows.h, "Mix", twice -- in numpy with wrapping uint64 arithmetic (what the GPU tests compare
every byte and the count with) and a sample at a time in Python ints (what the first is held to on the CPU).  The table is the
library's own carrier table (gpsiq.carrier_table()).  TEST INFRASTRUCTURE: nothing here is product code."""
import functools

import numpy as np

import gpsiq
from gpsiq.abi import MIX_ROTATED, MIX_STREAM, MIX_TONE, SC08

M64 = 2 ** 64
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


class Term:
    """A term of the contract with its source as an array: x [len, 2] int8 / int16 (sample 0 of the term first) or None for a tone;
    sweep = (period, offset), gate = (period, on, offset)."""

    def __init__(self, kind, gain, x=None, skip=0, phase0=0, step=0, rate=0, sweep=(0, 0), gate=(0, 0, 0)):
        self.kind, self.gain, self.x, self.skip = kind, int(gain), x, int(skip)
        self.phase0, self.step, self.rate, self.sweep, self.gate = int(phase0), int(step), int(rate), tuple(sweep), tuple(gate)

    @property
    def sample_size(self):
        return 0 if self.x is None else self.x.dtype.itemsize

    def mixterm(self, ptr=0):
        """the gpsiq.MixTerm of this term with its source at address ptr"""
        return gpsiq.MixTerm(kind=self.kind, sample_size=self.sample_size, src=int(ptr) or None, skip=self.skip, gain=self.gain, phase0=self.phase0 % M64,
                             step=self.step, rate=self.rate, sweep_period=self.sweep[0], sweep_offset=self.sweep[1], gate_period=self.gate[0],
                             gate_on=self.gate[1], gate_offset=self.gate[2])

    def advanced(self, done):
        """gpsiq_mix_advance restated: the term of a continuation `done` samples on"""
        t = Term(self.kind, self.gain, self.x, self.skip, self.phase0, self.step, self.rate, self.sweep, self.gate)
        if self.kind != MIX_TONE:
            t.skip = max(0, self.skip - done)
            t.x = self.x[max(0, done - self.skip):]
        return t


def _u(v):
    return np.uint64(int(v) % M64)


def mix_ref(nsamp, m0, terms, shift, qmax, out_dtype):
    """-> (out [nsamp, 2] of out_dtype, elements the clamp changed)"""
    cos, sin = table()
    n = np.arange(nsamp, dtype=np.uint64)
    with np.errstate(over="ignore"):
        m = n + _u(m0)
        acc = np.zeros((nsamp, 2), np.int64)
        for t in terms:
            gp, gon, goff = t.gate
            on = np.ones(nsamp, bool) if gp == 0 else ((m + _u(goff)) % np.uint64(gp)) < np.uint64(gon)
            x = np.zeros((nsamp, 2), np.int64)
            if t.kind != MIX_TONE:
                have = max(0, nsamp - t.skip)
                if have:
                    x[t.skip:] = t.x[:have]
            sp, so = t.sweep
            r = m if sp == 0 else (m + _u(so)) % np.uint64(sp)
            one = np.uint64(1)
            tri = np.where(r & one, r * ((r - one) >> one), (r >> one) * (r - one))
            theta = _u(t.phase0) + m * _u(t.step) + tri * _u(t.rate)
            idx = ((theta >> np.uint64(50)) & np.uint64(511)).astype(np.int64)
            c, s = cos[idx], sin[idx]
            if t.kind == MIX_STREAM:
                v = x
            elif t.kind == MIX_ROTATED:
                v = np.stack([x[:, 0] * c - x[:, 1] * s, x[:, 0] * s + x[:, 1] * c], axis=1)
            else:
                v = np.stack([c, s], axis=1)
            acc += np.int64(t.gain) * np.where(on[:, None], v, 0)
    y = acc if shift == 0 else (acc + (np.int64(1) << np.int64(shift - 1))) >> np.int64(shift)
    out = np.clip(y, -qmax, qmax)
    return out.astype(out_dtype), int(np.count_nonzero(out != y))


def mix_slow(nsamp, m0, terms, shift, qmax, out_dtype):
    """the contract a sample at a time in Python ints"""
    cos, sin = table()
    out = np.zeros((nsamp, 2), out_dtype)
    clipped = 0
    for n in range(nsamp):
        m = (m0 + n) % M64
        acc = [0, 0]
        for t in terms:
            gp, gon, goff = t.gate
            if gp and ((m + goff) % M64) % gp >= gon:
                continue
            xi = xq = 0
            if t.kind != MIX_TONE and n >= t.skip:
                xi, xq = int(t.x[n - t.skip, 0]), int(t.x[n - t.skip, 1])
            sp, so = t.sweep
            r = ((m + so) % M64) % sp if sp else m
            theta = (t.phase0 + m * t.step + (r * (r - 1) // 2) * t.rate) % (2 ** 59)
            c, s = int(cos[theta >> 50]), int(sin[theta >> 50])
            if t.kind == MIX_STREAM:
                v = (xi, xq)
            elif t.kind == MIX_ROTATED:
                v = (xi * c - xq * s, xi * s + xq * c)
            else:
                v = (c, s)
            acc[0] += t.gain * v[0]
            acc[1] += t.gain * v[1]
        for e in range(2):
            y = acc[e] if shift == 0 else (acc[e] + (1 << (shift - 1))) >> shift
            o = min(max(y, -qmax), qmax)
            clipped += o != y
            out[n, e] = o
    return out, clipped
