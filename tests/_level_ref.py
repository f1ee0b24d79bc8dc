"""numpy restatement of the output level contract (include/gpsiq_rows.h, "Output level"), independent of the library: Python / numpy
integers on top of tests/_noise_ref.py's noise and the oracle's noiseless int16 block.

    S = the noiseless int16 element       A = S + z       y = floor((A * mult + 32768) / 65536)       out = min(max(y, -qmax), qmax)
"""
import math

import numpy as np

import _noise_ref as nr


def stage(A, mult, qmax):
    """The stage on int64 values A (|A| < 2^19, mult < 2^24: the product fits int64 with room to spare; // is floor)."""
    A = np.asarray(A, dtype=np.int64)
    y = (A * np.int64(mult) + np.int64(32768)) // np.int64(65536)
    return np.clip(y, -int(qmax), int(qmax))


def level(clean16, z, mult, qmax, sample_size):
    """clean16: the noiseless int16 stream [nblocks, 2*nsamp] (the wrapped sums, as the int16 store keeps them); z: the noise
    [nblocks, nsamp, 2] as _noise_ref.noise gives it, or None.  Returns the stream in the format's element type."""
    S = np.asarray(clean16).astype(np.int64)
    A = S if z is None else S + np.asarray(z, dtype=np.int64).reshape(S.shape)
    return stage(A, mult, qmax).astype(np.int16 if sample_size == 2 else np.int8)


def composite_rms(gains, sigma):
    return math.sqrt(sigma * sigma + sum((250.0 * g) ** 2 / 2.0 for g in gains))


def level_mult(rms_in, rms_out):
    m = float(np.rint(65536.0 * rms_out / rms_in))
    return int(min(max(m, 1.0), 2.0 ** 24 - 1))


def table_values(sigma):
    """The 65 536 values z(u), u = 0 .. 65535, each drawn with probability 2^-16."""
    S, St = nr.tables(sigma)
    return nr.z_of(np.arange(65536, dtype=np.uint64), S, St)
