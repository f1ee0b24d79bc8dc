"""tests/_stap_beams_ref.py held to hand-made cases, to tests/_stap_ref.py and tests/_cfilter_ref.py, and the host arithmetic of the
call -- gpsiq_stap_beam_weights (libgpsiq_rows.so; no device) -- held to gpsiq_stap_weights bit for bit, to the contract's properties
per beam and to its refusals; and the scene of four satellites through the restatements: every beam keeps its own satellite."""
import ctypes as C

import numpy as np
import pytest

import _cfilter_ref as cr
import _stap_beams_ref as br
import _stap_ref as sr
import gpsiq

PAIRS = pytest.mark.parametrize("in_size,out_size", [(1, 1), (1, 2), (2, 1), (2, 2)], ids=["8to8", "8to16", "16to8", "16to16"])


def test_two_beams_by_hand():
    """two elements, two taps, shift 0: beam 0 is x_0(n) + j x_1(n - 1), beam 1 is -x_1(n); no head, then a head"""
    x0 = np.array([[1, 2], [3, 4], [5, 6]], np.int8)
    x1 = np.array([[7, 8], [9, 10], [11, 12]], np.int8)
    w = np.zeros((2, 2, 2, 2), np.int16)
    w[0, 0, 0] = (1, 0)
    w[0, 1, 1] = (0, 1)
    w[1, 1, 0] = (-1, 0)
    outs, counts = br.beams_ref([x0, x1], None, w, 0, 2)
    # j (I + j Q) = -Q + j I
    assert outs[0].tolist() == [[1, 2], [3 - 8, 4 + 7], [5 - 10, 6 + 9]] and outs[1].tolist() == (-x1.astype(int)).tolist() and not counts.any()
    outs, _ = br.beams_ref([x0, x1], [None, np.array([[20, 30]], np.int8)], w, 0, 2)
    assert outs[0].tolist()[0] == [1 - 30, 2 + 20]
    for a, b in zip(outs, br.beams_scalar([x0, x1], [None, np.array([[20, 30]], np.int8)], w, 0, 2)[0]):
        assert np.array_equal(a, b)


@PAIRS
def test_one_beam_is_the_combiner_and_the_two_statements_agree(in_size, out_size):
    rng = np.random.default_rng(10 * in_size + out_size)
    for nelem, ntaps, nbeams, shift in ((1, 1, 1, 0), (2, 4, 3, 9), (3, 3, 8, 14), (4, 5, 2, 24)):
        xs = sr.streams(rng, nelem, 40, in_size)
        heads = [None if e % 2 else h for e, h in enumerate(sr.streams(rng, nelem, ntaps - 1, in_size))]
        lim = min(65535 // (2 * nelem * ntaps), 32767) if shift else 2
        w = rng.integers(-lim, lim + 1, size=(nbeams, nelem, ntaps, 2)).astype(np.int16)
        outs, counts = br.beams_ref(xs, heads, w, shift, out_size)
        souts, scounts = br.beams_scalar(xs, heads, w, shift, out_size)
        assert len(outs) == nbeams and np.array_equal(counts, scounts) and counts.dtype == np.uint64
        for b in range(nbeams):
            y, c = sr.combine_ref(xs, heads, w[b], shift, out_size)
            assert np.array_equal(outs[b], y) and np.array_equal(souts[b], y) and counts[b] == c


@PAIRS
def test_beams_do_not_leak_into_each_other(in_size, out_size):
    """beam 0 at the bound with every output clamping beside beam 1 all zeros, and the reverse"""
    lo = -128 if in_size == 1 else -32768
    xs = [np.full((33, 2), lo, np.int8 if in_size == 1 else np.int16) for _ in range(2)]
    w = np.zeros((2, 2, 4, 2), np.int16)
    w[0, :, :, 0] = 65535 // 8                                          # real weights: accI = accQ = lo * sum re, from the first sample on
    w[0, 0, 0, 0] += 65535 - int(w[0].sum())
    assert int(np.abs(w[0].astype(int)).sum()) == 65535
    for order in ((0, 1), (1, 0)):
        outs, counts = br.beams_ref(xs, None, w[list(order)], 0, out_size)
        loud, quiet = order.index(0), order.index(1)
        assert counts[loud] == 2 * 33 and counts[quiet] == 0 and not outs[quiet].any() and (np.abs(outs[loud].astype(int)) == (127 if out_size == 1 else 32767)).all()
        souts, scounts = br.beams_scalar(xs, None, w[list(order)], 0, out_size)
        assert np.array_equal(counts, scounts) and all(np.array_equal(a, b) for a, b in zip(outs, souts))


@PAIRS
def test_one_element_and_one_beam_is_the_complex_filter(in_size, out_size):
    rng = np.random.default_rng(3)
    for ntaps, shift in ((1, 0), (5, 12), (8, 20)):
        (x,), (h,) = sr.streams(rng, 1, 200, in_size), sr.streams(rng, 1, ntaps - 1, in_size)
        lim = 65535 // (2 * ntaps) if shift else 1
        taps = rng.integers(-min(lim, 32767), min(lim, 32767) + 1, size=(ntaps, 2)).astype(np.int16)
        (y,), (c,) = br.beams_ref([x], [h], taps[None, None], shift, out_size)
        f, fc = cr.cfilter_ref(x, h, taps, shift, 1, 0, out_size)
        assert np.array_equal(y, f) and c == fc


def test_max_entry_is_what_the_planes_must_hold():
    w = np.zeros((2, 1, 2, 2), np.int16)
    w[1, 0, 1] = (-32768, -5)
    assert br.max_entry(w) == 5
    w[0, 0, 0, 1] = -32768
    assert br.max_entry(w) == 32768 > br.MAX_ENTRY


# ---- gpsiq_stap_beam_weights -------------------------------------------------------------------------------------------------------------
def _sample_cov(nelem, ntaps, seed, nsamp=4000):
    rng = np.random.default_rng(seed)
    j = 40.0 * (rng.standard_normal(nsamp + 2) + 1j * rng.standard_normal(nsamp + 2))
    xs = []
    for e in range(nelem):
        x = np.exp(2j * np.pi * 0.23 * e) * j[2:] + 0.6 * np.exp(2j * np.pi * 0.61 * e * e) * j[:nsamp] + 8.0 * (rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp))
        xs.append(np.stack([np.rint(x.real), np.rint(x.imag)], axis=1).astype(np.int16))
    cov = sr.cov_ref(xs, None, ntaps)
    return cov, (cov[:, :, 0] + 1j * cov[:, :, 1]) / float(nsamp), nsamp


STEERS = np.array([[0.0, 0.2, 0.63, 0.41], [0.5, 0.25, 0.0, 0.75], [0.11, 0.93, 0.37, 0.58], [0.0, 0.0, 0.0, 0.0], [0.9, 0.1, 0.3, 0.7],
                   [0.05, 0.5, 0.45, 0.95], [0.33, 0.66, 0.99, 0.32], [0.125, 0.25, 0.375, 0.5]])


@pytest.mark.parametrize("nelem,ntaps", [(1, 1), (2, 4), (4, 2), (3, 3), (4, 8)])
def test_every_beam_is_stap_weights_bit_for_bit_and_keeps_the_contracts_properties(nelem, ntaps):
    cov, rn, nsamp = _sample_cov(nelem, ntaps, 500 + nelem + ntaps)
    kk, shift = nelem * ntaps, 11
    for nbeams, ref_tap, loading in ((1, 0, 0.0), (3, ntaps - 1, 0.02), (8, ntaps // 2, 0.0)):
        steers = STEERS[:nbeams, :nelem]
        w = gpsiq.stap_beam_weights(cov, nsamp, nelem, ntaps, steers, ref_tap=ref_tap, loading=loading, shift=shift)
        assert w.shape == (nbeams, nelem, ntaps, 2) and w.dtype == np.int16
        rl = rn + loading * (np.trace(rn).real / kk) * np.eye(kk)
        for b in range(nbeams):
            one = gpsiq.stap_weights(cov, nsamp, nelem, ntaps, steer=steers[b], ref_tap=ref_tap, loading=loading, shift=shift)
            assert np.array_equal(w[b], one), b
            c = np.zeros(kk, np.complex128)
            c[np.arange(nelem) * ntaps + ref_tap] = np.exp(2j * np.pi * steers[b])
            wk = w[b].reshape(-1, 2).astype(np.int64)
            # property 2: only rounding is left in the constraint
            assert abs(((wk[:, 0] + 1j * wk[:, 1]) * c).sum() - (1 << shift)) <= kk / np.sqrt(2.0) + 1e-6
            # property 3: v^H Rn v = 1 / (c^H Rn^-1 c) is the minimum over the constraint, which u = c / nelem meets too
            v = (wk[:, 0] - 1j * wk[:, 1]) / float(1 << shift)
            u = c / nelem
            slack = 2 * np.abs(v).sum() * np.abs(rl).max() * kk * 0.7072 / (1 << shift)
            assert (v.conj() @ rl @ v).real <= (u.conj() @ rl @ u).real + slack


def _raw(cov, nelem, ntaps, nsamp, steers, nbeams, ref_tap, loading, shift, fill=0x5A5A):
    """the C call itself on a buffer of sentinels -> (return code, int16 [nbeams, K, 2])"""
    w = np.full((max(nbeams, 1) * nelem * ntaps + 4, 2), fill, dtype=np.int16)
    cov = np.ascontiguousarray(cov, dtype=np.int64)
    st = None if steers is None else np.ascontiguousarray(steers, dtype=np.float64)
    rc = gpsiq._stap_beam_weights(cov.ctypes.data_as(C.c_void_p), nelem, ntaps, nsamp, None if st is None else st.ctypes.data_as(C.c_void_p), nbeams, ref_tap,
                                  loading, shift, w.ctypes.data_as(C.c_void_p))
    return rc, w


def test_weights_refusals_and_what_a_refusal_leaves_unwritten():
    cov, _, nsamp = _sample_cov(2, 4, 300)
    good = STEERS[:3, :2]
    ok, w = _raw(cov, 2, 4, nsamp, good, 3, 0, 0.0, 11)
    assert ok == 0 and (w[24:] == 0x5A5A).all() and not (w[:24] == 0x5A5A).all(axis=1).any()
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.stap_beam_weights(cov, 0, 2, 4, good)
    E_ARG = e.value.code
    for kw in (dict(loading=-0.1), dict(loading=float("nan")), dict(shift=-1), dict(shift=25), dict(ref_tap=-1), dict(ref_tap=4)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.stap_beam_weights(cov, nsamp, 2, 4, good, **kw)
        assert e.value.code == E_ARG, kw
    for nbeams, steers in ((0, good), (9, np.zeros((9, 2))), (2, None)):
        assert _raw(cov, 2, 4, nsamp, steers, nbeams, 0, 0.0, 11)[0] == E_ARG
    with pytest.raises(gpsiq.GpsiqError):
        gpsiq.stap_beam_weights(cov, nsamp, 2, 4, np.zeros((2, 3)))     # steering phases of another shape
    # beam 1 is refused after beam 0 succeeded: beam 0 stands, nothing is written for beams 1 and 2
    bad = good.copy()
    bad[1, 1] = float("nan")
    rc, w = _raw(cov, 2, 4, nsamp, bad, 3, 0, 0.0, 11)
    assert rc == E_ARG and np.array_equal(w[:8].reshape(2, 4, 2), gpsiq.stap_weights(cov, nsamp, 2, 4, steer=good[0], shift=11)) and (w[8:] == 0x5A5A).all()
    # the same with GPSIQ_E_RANGE: three equal elements at shift 16 round to 3 * 21845 = 65535 towards phase 0 and pass; towards an
    # eighth of a cycle every weight has re = im and the sum is 92 thousand
    eye3 = np.zeros((3, 3, 2), np.int64)
    eye3[np.arange(3), np.arange(3), 0] = 1000
    st = np.array([[0.0, 0.0, 0.0], [0.125, 0.125, 0.125], [0.0, 0.0, 0.0]])
    rc, w = _raw(eye3, 3, 1, 1000, st, 3, 0, 0.0, 16)
    assert rc not in (0, E_ARG) and w[:3].tolist() == [[21845, 0]] * 3 and (w[3:] == 0x5A5A).all()
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.stap_weights(eye3, 1000, 3, 1, steer=st[1], shift=16)
    assert e.value.code == rc
    assert gpsiq.STAP_MAX_BEAMS == br.MAX_BEAMS == 8


# ---- the scene -------------------------------------------------------------------------------------------------------------------------
def test_every_satellite_keeps_its_prompt_behind_its_own_beam_in_the_scene(capsys):
    """The four beams' weights, computed from the jammed covariance, applied to the four CLEAN elements through the restatements.
    Satellite s reaches element e as its element-0 stream times c_(s,e), so behind beam b it is that stream through the FIR
    g[t] = sum over e of w_b[e][t] c_(s,e) / 2^shift; for its own beam g[0] is 1 to the constraint's rounding, and a replica t samples
    late correlates with the code by its autocorrelation rho(t): tests/test_gpu_stap_signal.py's argument, per beam.  The scene's
    directions and delay are chosen so that every beam keeps more than half by that bound."""
    sc = br.scene()
    nsat = len(br.PRNS)
    assert sc["w"].shape == (nsat, br.NELEM, br.NTAPS, 2) and (sc["prompt_clean"] > 0).all()
    for b in range(nsat):
        g = br.fir_seen(sc["w"][b], sc["steers"][b], br.SHIFT)
        assert abs(g[0] - 1.0) <= (br.NELEM * br.NTAPS / np.sqrt(2.0) + 1e-6) / (1 << br.SHIFT)
        assert sc["keep"][b] > 0.5
        assert sc["prompt_beams"][b, b] >= sc["keep"][b] * sc["prompt_clean"][b], (b, sc["prompt_beams"][b, b], sc["keep"][b], sc["prompt_clean"][b])
    with capsys.disabled():
        print("\nkeep per beam", np.round(sc["keep"], 3).tolist(), "; own beam over clean", np.round(np.diag(sc["prompt_beams"]) / sc["prompt_clean"], 3).tolist())
        print("behind the beam steered at satellite 0, every satellite's prompt over its prompt in the clean element (what one stap_combine call "
              "gives a receiver):", np.round(sc["prompt_beams"][0] / sc["prompt_clean"], 3).tolist())
