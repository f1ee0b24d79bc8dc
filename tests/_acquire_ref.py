"""numpy restatement of gpsiq_acquire's contract (include/gpsiq_rows.h, "Acquisition").  Codes and the unit table come from the
oracle, where tests/_despread_ref.py takes its replica from; the carrier index is 64-bit wrapping integer arithmetic (2^59 divides
2^64, so the wrap does not touch the residue), the correlations are a float64 matrix product in which every partial sum is an
integer below 2^44 (|y| <= 32768 * 355 < 2^23.5, ncoh <= 2^20) and therefore exact, and the power is the contract's sequential
float64 loop.  Nothing else restates the search.  TEST INFRASTRUCTURE."""
import numpy as np

from gpsiq.abi import ACQ_PEAK_DTYPE, DESPREAD_SUM_DTYPE

MASK59 = (1 << 59) - 1


def sampled_code(orc, prn, code_step, ncoh):
    """int64 [ncoh]: +1 where chip ((n * code_step) >> 56) % 1023 is 0, -1 where it is 1 (exact Python integers)"""
    chips = orc.codegen(int(prn)).astype(np.int64)
    idx = [((n * int(code_step)) >> 56) % 1023 for n in range(ncoh)]
    return 1 - 2 * chips[idx]


def carrier_index(step, count):
    """int64 [count]: ((m * step) mod 2^59) >> 50 for m = 0 .. count - 1, step any Python integer"""
    m = np.arange(count, dtype=np.uint64)
    return (((m * np.uint64(int(step) % (1 << 64))) & np.uint64(MASK59)) >> np.uint64(50)).astype(np.int64)


def wipe(orc, stream, count, carr_step0, carr_step_inc, ndopp):
    """stream: integer array of interleaved I, Q -> (yi, yq) int64 [ndopp][count] of its first `count` samples"""
    s, c = orc.tables()
    s, c = s.astype(np.int64), c.astype(np.int64)
    x = np.asarray(stream).astype(np.int64).reshape(-1, 2)[:count]
    yi = np.zeros((ndopp, count), dtype=np.int64)
    yq = np.zeros((ndopp, count), dtype=np.int64)
    for d in range(ndopp):
        idx = carrier_index(int(carr_step0) + d * int(carr_step_inc), count)
        yi[d] = x[:, 0] * c[idx] + x[:, 1] * s[idx]
        yq[d] = x[:, 1] * c[idx] - x[:, 0] * s[idx]
    return yi, yq


def digits(y, nd):
    """balanced base-256 digits, least significant first: int64 [nd, ...] with y = sum d_i 256^i, and what is left over (0 if nd is enough)"""
    y = np.asarray(y, dtype=np.int64).copy()
    out = []
    for _ in range(nd):
        d = ((y + 128) & 255) - 128
        out.append(d)
        y = (y - d) >> 8
    return np.stack(out), y


def acquire(orc, stream, prns, code_step, carr_step0, carr_step_inc, ndopp, nshift, ncoh, nnoncoh=1, hop=None):
    """-> (peaks ACQ_PEAK_DTYPE [nprn][ndopp], power float64 [nprn][ndopp][nshift], corr DESPREAD_SUM_DTYPE [nprn][ndopp][nnoncoh][nshift])"""
    hop = ncoh if hop is None else hop
    span = (nshift - 1) + (nnoncoh - 1) * hop + ncoh
    assert 2 * span <= np.asarray(stream).size
    yi, yq = wipe(orc, stream, span, carr_step0, carr_step_inc, ndopp)
    ca = np.stack([sampled_code(orc, p, code_step, ncoh) for p in prns]).astype(np.float64)          # [nprn][ncoh]
    corr = np.zeros((len(prns), ndopp, nnoncoh, nshift), dtype=DESPREAD_SUM_DTYPE)
    win = np.lib.stride_tricks.sliding_window_view
    for d in range(ndopp):
        for k in range(nnoncoh):
            lo, hi = k * hop, k * hop + nshift - 1 + ncoh
            for y, f in ((yi, "i"), (yq, "q")):
                x = win(y[d, lo:hi].astype(np.float64), ncoh) @ ca.T                                   # [nshift][nprn], exact integers
                corr[f][:, d, k, :] = x.T.astype(np.int64)
    power = np.zeros((len(prns), ndopp, nshift), dtype=np.float64)
    for k in range(nnoncoh):                                                                           # the contract's order
        xi, xq = corr["i"][:, :, k, :].astype(np.float64), corr["q"][:, :, k, :].astype(np.float64)
        power = power + (xi * xi + xq * xq)
    peaks = np.zeros((len(prns), ndopp), dtype=ACQ_PEAK_DTYPE)
    at = power.argmax(axis=2)                                                                          # the first of equals
    peaks["shift"] = at
    peaks["power"] = np.take_along_axis(power, at[:, :, None], axis=2)[:, :, 0]
    return peaks, power, corr


def carrier_index_from(step, first, count):
    """int64 [count]: ((m * step) mod 2^59) >> 50 for the ABSOLUTE samples m = first .. first + count - 1 (64-bit wrapping product)"""
    m = np.arange(count, dtype=np.uint64) + np.uint64(first)
    return (((m * np.uint64(int(step) % (1 << 64))) & np.uint64(MASK59)) >> np.uint64(50)).astype(np.int64)


def acquire_windows(orc, windows, first, prns, code_step, carr_step0, carr_step_inc, ndopp, nshift, ncoh):
    """The search of a span too long to hold densely, from its dwell windows alone: windows[k] the elements (interleaved I, Q) of samples
    [first[k], first[k] + nshift - 1 + ncoh) of the span, first[k] = k * hop the window's ABSOLUTE first sample -- the carrier index of a
    sample is taken at its absolute m, everything else is local to the window.  No sample outside the windows is an input of the
    contract's sums.  -> acquire()'s (peaks, power, corr)."""
    s, c = orc.tables()
    s, c = s.astype(np.int64), c.astype(np.int64)
    ca = np.stack([sampled_code(orc, p, code_step, ncoh) for p in prns]).astype(np.float64)
    width = nshift - 1 + ncoh
    corr = np.zeros((len(prns), ndopp, len(windows), nshift), dtype=DESPREAD_SUM_DTYPE)
    for k, (w, m0) in enumerate(zip(windows, first)):
        x = np.asarray(w).astype(np.int64).reshape(-1, 2)
        assert len(x) == width
        for d in range(ndopp):
            idx = carrier_index_from(int(carr_step0) + d * int(carr_step_inc), int(m0), width)
            yi, yq = x[:, 0] * c[idx] + x[:, 1] * s[idx], x[:, 1] * c[idx] - x[:, 0] * s[idx]
            for y, f in ((yi, "i"), (yq, "q")):
                corr[f][:, d, k, :] = (np.lib.stride_tricks.sliding_window_view(y.astype(np.float64), ncoh) @ ca.T).T.astype(np.int64)
    power = np.zeros((len(prns), ndopp, nshift), dtype=np.float64)
    for k in range(len(windows)):
        xi, xq = corr["i"][:, :, k, :].astype(np.float64), corr["q"][:, :, k, :].astype(np.float64)
        power = power + (xi * xi + xq * xq)
    peaks = np.zeros((len(prns), ndopp), dtype=ACQ_PEAK_DTYPE)
    at = power.argmax(axis=2)
    peaks["shift"] = at
    peaks["power"] = np.take_along_axis(power, at[:, :, None], axis=2)[:, :, 0]
    return peaks, power, corr


def acquire_direct(orc, stream, prn, code_step, step, s, k, hop, ncoh):
    """one (Xi, Xq) in Python integers, sample by sample: what the matrix product above is held against"""
    sn, cs = orc.tables()
    x = np.asarray(stream).astype(np.int64).reshape(-1, 2)
    ca = sampled_code(orc, prn, code_step, ncoh)
    xi = xq = 0
    for n in range(ncoh):
        m = s + k * hop + n
        idx = ((m * int(step)) % (1 << 59)) >> 50
        i, q, rc, rs = int(x[m, 0]), int(x[m, 1]), int(cs[idx]), int(sn[idx])
        xi += (i * rc + q * rs) * int(ca[n])
        xq += (q * rc - i * rs) * int(ca[n])
    return xi, xq


def acquire_direct_window(orc, window, first, prn, code_step, step, s, ncoh):
    """acquire_direct for one dwell given as its window (acquire_windows' layout): the carrier at the absolute sample first + s + n"""
    sn, cs = orc.tables()
    x = np.asarray(window).astype(np.int64).reshape(-1, 2)
    ca = sampled_code(orc, prn, code_step, ncoh)
    xi = xq = 0
    for n in range(ncoh):
        idx = (((int(first) + s + n) * int(step)) % (1 << 59)) >> 50
        i, q, rc, rs = int(x[s + n, 0]), int(x[s + n, 1]), int(cs[idx]), int(sn[idx])
        xi += (i * rc + q * rs) * int(ca[n])
        xq += (q * rc - i * rs) * int(ca[n])
    return xi, xq


def steps(fs, f0_hz, df_hz):
    """gpsiq_acquire_steps' formulas"""
    return (int(np.rint(1.023e6 / fs * 2.0 ** 56)), int(np.rint(f0_hz / fs * 2.0 ** 59)), int(np.rint(df_hz / fs * 2.0 ** 59)))


def decide(power, guard):
    """gpsiq_acquire_decide's rule: (bin, shift, ratio), or None where the library answers GPSIQ_E_RANGE"""
    power = np.asarray(power, dtype=np.float64)
    d, s = np.unravel_index(int(power.argmax()), power.shape)                                          # row-major: lowest d, then lowest s
    far = np.abs(np.arange(power.shape[1]) - s) > guard
    if not far.any() or not power[:, far].max() > 0.0:
        return None
    return int(d), int(s), float(power[d, s] / power[:, far].max())


# ---- the closed loop: tests/_despread_ref.py's LOOP, both satellites rendered (tests/test_acquire_ref.py, tests/test_gpu_acquire.py) ----
SEARCH = dict(ncoh=2560, hop=2600, nnoncoh=4, f0=-5000.0, df=500.0, ndopp=21, nshift=2600, guard=3, prns=(7, 19, 3, 28))


def loop_descriptors():
    """CHAN_DTYPE [1][2]: the first block of LOOP with BOTH satellites at LOOP's gain, i.e. both at LOOP's C/N0"""
    import _despread_ref as dr
    d = dr.loop_descriptors()[:1].copy()
    d["gain"][:, 1] = dr.LOOP["gain"]
    return d


def expected_cell(ch, fs):
    """(bin, shift as a real number) a channel of the first block should be found at: the bin nearest f_carr, and the sample at
    which its code reaches chip 0"""
    S = SEARCH
    return int(np.rint((ch["f_carr"] - S["f0"]) / S["df"])), ((1023.0 - ch["code_phase"]) % 1023.0) / (ch["f_code"] / fs)
