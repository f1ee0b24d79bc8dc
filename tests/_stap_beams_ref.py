"""gpsiq_stap_beams restated from its contract (include/gpsiq_rows.h, "Space-time array", "Several beams from one pass"): beam b is
gpsiq_stap_combine with w[b], so the restatement is a loop of tests/_stap_ref.py's combine_ref -- imported, and left alone -- with a
scalar twin in Python integers for the by-hand cases, and the scene the call exists for: four elements, four satellites, a broadband
jammer that arrives twice.  TEST INFRASTRUCTURE: the restatements read no line of the library; the scene takes its descriptors and
its steering phases from the library's host arithmetic, as tests/test_gpu_stap_signal.py does.

Streams, heads and rows are tests/_stap_ref.py's; weights are [nbeams, nelem, ntaps, 2] (re, im)."""
import functools
import math

import numpy as np

import _stap_ref as sr

MAX_BEAMS = 8
MAX_ENTRY = 127 * 256 + 127            # the largest of re, +im, -im that splits into two signed bytes


def _weights(w, nelem):
    w = np.asarray(w)
    assert w.ndim == 4 and 1 <= w.shape[0] <= MAX_BEAMS and w.shape[1] == nelem and w.shape[3] == 2
    return w


def beams_ref(xs, heads, w, shift, out_size):
    """-> (list of nbeams outputs int8 / int16 [n, 2], uint64 [nbeams] counts)"""
    w = _weights(w, len(xs))
    outs, counts = [], []
    for wb in w:
        y, c = sr.combine_ref(xs, heads, wb, shift, out_size)
        outs.append(y)
        counts.append(c)
    return outs, np.array(counts, dtype=np.uint64)


def beams_scalar(xs, heads, w, shift, out_size):
    """The same contract written out once more, a beam, a sample and a term at a time, in Python integers."""
    w = _weights(w, len(xs))
    xs = [np.asarray(x).reshape(-1, 2) for x in xs]
    heads = [None] * len(xs) if heads is None else [None if h is None else np.asarray(h).reshape(-1, 2) for h in heads]
    ntaps = w.shape[2]
    qmax = 127 if out_size == 1 else 32767
    outs, counts = [], []
    for b in range(w.shape[0]):
        assert sum(abs(int(v)) for v in w[b].ravel()) <= sr.WEIGHT_SUM
        rows, clipped = [], 0
        for n in range(len(xs[0])):
            acc = [0, 0]
            for e in range(len(xs)):
                for t in range(ntaps):
                    re, im = int(w[b][e][t][0]), int(w[b][e][t][1])
                    i, q = sr.x_at(xs[e], heads[e], ntaps, n - t)
                    acc[0] += re * i - im * q
                    acc[1] += re * q + im * i
            row = []
            for a in acc:
                y = a if shift == 0 else (a + 2 ** (shift - 1)) // 2 ** shift
                o = min(max(y, -qmax), qmax)
                clipped += o != y
                row.append(o)
            rows.append(row)
        outs.append(np.array(rows, dtype=np.int8 if out_size == 1 else np.int16).reshape(-1, 2))
        counts.append(clipped)
    return outs, np.array(counts, dtype=np.uint64)


def max_entry(w):
    """the largest of re, +im, -im over all beams: what decides whether the matrix kernel's digit planes can hold the weights"""
    w = np.asarray(w).astype(np.int64)
    return int(max(w[..., 0].max(), w[..., 1].max(), (-w[..., 1]).max()))


def weights_at_the_bound(nelem, ntaps, signs):
    """one beam [nelem, ntaps, 2] with sum |re| + |im| = 65535 exactly (65534 for one row, both positive), every re of sign signs[0]
    and every im of sign signs[1], and every entry inside the digit planes' range where K > 1"""
    rows = nelem * ntaps
    if rows == 1:
        re = 32767 if signs[0] > 0 else -32768
        im = 32767 if signs[1] > 0 else -32768 if signs[0] > 0 else -32767
        w = np.array([[re, im]], np.int64)
    else:
        w = np.full((rows, 2), 65535 // (2 * rows), np.int64)
        w[0, 0] += 65535 - int(w.sum())
        w[:, 0] *= signs[0]
        w[:, 1] *= signs[1]
    assert int(np.abs(w).sum()) in (65535, 65534) and w.min() >= -32768 and w.max() <= 32767
    return w.astype(np.int16).reshape(nelem, ntaps, 2)


# ---- the scene: four elements, four satellites, a broadband jammer and its echo ---------------------------------------------------------
# Four elements on a half-wavelength square (tests/_array_ref.py, SQUARE; element 0 at the origin, so every arrival has phase 0 there),
# four satellites from four directions in the four channel slots, each under the noise (gain 0.2: amplitude 50 against a noise sigma of
# 101 a component at 55 dB-Hz), independent receiver noise per element, and ONE white jammer stream that gpsiq_mix adds to every element
# twice: directly from one direction and again D samples later from another (tests/test_gpu_stap_signal.py's construction and gains).
# Two blocks of tests/_despread_ref.py's 2.6 Msps closed loop.  D = 3: the weights that cancel the reflection sit three taps late, where
# the code's autocorrelation is 1 / 1023 of the prompt at 2.6 Msps, so what a beam's taps take from its own satellite is decided by the
# taps at 1 and 2 samples, which only the noise fills.
NB, NELEM, NTAPS, D, SHIFT = 2, 4, 4, 3, 12
PRNS = (7, 19, 3, 28)
GAIN, CN0 = 0.2, 55.0
SATS = ((30.0, 50.0), (120.0, 35.0), (210.0, 65.0), (300.0, 25.0))      # azimuth, elevation in degrees
JAM_DIRECT, JAM_ECHO = (75.0, 5.0), (250.0, 12.0)
JAM_SIGMA = 4500.0
MIX_SHIFT, G_STREAM, G_DIRECT, G_ECHO = 10, 1 << 10, 4, 3


def rho(t, fs):
    """the C/A code's autocorrelation t samples late, as a share of the prompt: the triangle, and at most 1 / 1023 beyond a chip"""
    return max(1.0 - t * 1.023e6 / fs, 1.0 / 1023.0)


def fir_seen(w, steer, shift):
    """g[t] = sum over e of w[e][t] c_e / 2^shift: the FIR a beam's weights [nelem, ntaps, 2] present to an arrival with phases steer"""
    c = np.exp(2j * np.pi * np.asarray(steer, dtype=np.float64))
    w = np.asarray(w).astype(np.int64)
    return ((w[:, :, 0] + 1j * w[:, :, 1]) * c[:, None]).sum(axis=0) / float(1 << shift)


def keep_of(g, fs):
    """tests/test_gpu_stap_signal.py's argument: the in-phase prompt keeps at least 0.95 - sum over t >= 1 of |g[t]| rho(t) of its size"""
    return 0.95 - sum(abs(g[t]) * rho(t, fs) for t in range(1, len(g)))


@functools.lru_cache(maxsize=None)
def scene():
    """the restatements' side of the whole chain, computed once: descriptors per element, clean, noisy and jammed streams, the mix terms,
    the covariance, the weights of the four beams, the beams of the jammed and of the clean elements, and every satellite's prompt in
    the clean element 0 and behind every beam of the clean elements"""
    import _array_ref as ar
    import _despread_ref as dr
    import _mix_ref as mr
    import _noise_ref as nr
    import _oracle
    import gpsiq
    from gpsiq.abi import MIX_ROTATED, MIX_STREAM, SC16
    from gpsiq.scenario import synth_blocks
    L = dr.LOOP
    ns, seg, fs = L["nsamp"], L["seg_len"], L["fs"]
    n = NB * ns
    orc = _oracle.load_oracle()
    sigma = gpsiq.noise_sigma_for_cn0(CN0, GAIN, fs)
    desc = synth_blocks(NB, len(PRNS), seed=45)
    for k, prn in enumerate(PRNS):
        desc["prn"][:, k], desc["gain"][:, k] = prn, GAIN
    rad = math.pi / 180.0
    steers = np.stack([gpsiq.array_steer(ar.SQUARE, az * rad, el * rad) for az, el in SATS])          # [satellite, element]
    jam_steer = [gpsiq.array_steer(ar.SQUARE, az * rad, el * rad) for az, el in (JAM_DIRECT, JAM_ECHO)]
    assert not steers[:, 0].any()
    rng = np.random.default_rng(0xBEA35)
    jam = np.clip(np.rint(rng.normal(0.0, JAM_SIGMA, size=(n, 2))), -32767, 32767).astype(np.int16)
    q, clean, noisy, jammed, terms = [], [], [], [], []
    for e in range(NELEM):
        qe, _ = gpsiq.quantize_blocks(gpsiq.array_element(desc, steers[:, e]), fs, ns)
        c = np.stack([orc.block_fixed(qe[b], ns, SC16) for b in range(NB)])
        x = nr.add_noise16(c, nr.noise(L["seed"] + e, sigma, 0, NB, ns)).reshape(-1, 2)
        t = [mr.Term(MIX_STREAM, G_STREAM, x), mr.Term(MIX_ROTATED, G_DIRECT, jam, phase0=int(round(jam_steer[0][e] * 2 ** 59))),
             mr.Term(MIX_ROTATED, G_ECHO, jam, skip=D, phase0=int(round(jam_steer[1][e] * 2 ** 59)))]
        y, clipped = mr.mix_ref(n, 0, t, MIX_SHIFT, 32767, np.int16)
        assert clipped == 0
        q.append(qe); clean.append(c.reshape(-1, 2)); noisy.append(x); jammed.append(y); terms.append(t)
    cov = sr.cov_ref(jammed, None, NTAPS)
    w = gpsiq.stap_beam_weights(cov, n, NELEM, NTAPS, steers, ref_tap=0, shift=SHIFT)
    beams_jammed = beams_ref(jammed, None, w, SHIFT, 2)
    beams_clean = beams_ref(clean, None, w, SHIFT, 2)
    assert not beams_jammed[1].any() and not beams_clean[1].any()

    def prompts(stream):
        """the mean in-phase prompt of every satellite in a stream [n, 2], against element 0's descriptors"""
        sums, _ = dr.despread(orc, q[0], np.asarray(stream).reshape(NB, 2 * ns), ns, seg)
        return np.array([sums["i"][:, k].astype(np.int64).mean() for k in range(len(PRNS))])

    return dict(ns=ns, seg=seg, fs=fs, n=n, sigma=sigma, seed=L["seed"], steers=steers, q=q, clean=clean, noisy=noisy, jammed=jammed, terms=terms,
                jam=jam, cov=cov, w=w, beams_jammed=beams_jammed, beams_clean=beams_clean, prompt_clean=prompts(clean[0]),
                prompt_beams=np.stack([prompts(y) for y in beams_clean[0]]),       # [beam, satellite]
                keep=np.array([keep_of(fir_seen(w[b], steers[b], SHIFT), fs) for b in range(len(PRNS))]))
