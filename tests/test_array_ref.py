"""The restatements of gpsiq_array_cov / gpsiq_array_combine (tests/_array_ref.py) held to hand-made cases and to each other, and the
host arithmetic of the stage -- gpsiq_array_steer, gpsiq_array_weights (libgpsiq_rows.so; no device) -- held to its contract
(include/gpsiq_rows.h, "Array"): properties, not bits."""
import numpy as np
import pytest

import gpsiq
import _array_ref as ar
import _cfilter_ref as cr


def test_covariance_by_hand():
    x0 = np.array([[1, 2], [3, -4], [-5, 6]])
    x1 = np.array([[7, -8], [9, 10], [-11, -12]])
    r = ar.cov_ref([x0, x1])
    # R[0][0] = 1+4 + 9+16 + 25+36; R[0][1]: re = sum Ia Ib + Qa Qb, im = sum Qa Ib - Ia Qb
    assert r[0, 0].tolist() == [91, 0] and r[1, 1].tolist() == [64 + 49 + 81 + 100 + 121 + 144, 0]
    assert r[0, 1].tolist() == [(7 - 16) + (27 - 40) + (55 - 72), (14 + 8) + (-36 - 30) + (-66 - 60)]
    assert r[1, 0].tolist() == [r[0, 1, 0], -r[0, 1, 1]]
    assert r.tolist() == ar.cov_scalar([x0, x1])


@pytest.mark.parametrize("in_size", [1, 2])
def test_covariance_is_hermitian_and_the_two_statements_agree(in_size):
    rng = np.random.default_rng(11 + in_size)
    for kind in ("random", "extremes"):
        xs = ar.streams(rng, 5, 37, in_size, kind)
        r = ar.cov_ref(xs, chunk=16)
        assert r.tolist() == ar.cov_scalar(xs)
        assert np.array_equal(r[:, :, 0], r[:, :, 0].T) and np.array_equal(r[:, :, 1], -r[:, :, 1].T)
        assert not r[np.arange(5), np.arange(5), 1].any() and (r[np.arange(5), np.arange(5), 0] >= 0).all()


def test_combine_by_hand():
    x0 = np.array([[1, 2], [3, -4], [-5, 6]])
    x1 = np.array([[7, -8], [9, 10], [-11, -12]])
    w = np.array([[2, 1], [-1, 3]])                                    # 2 + j, -1 + 3j
    out, clipped = ar.combine_ref([x0, x1], w, 0, 2)
    # (2 + j)(1 + 2j) + (-1 + 3j)(7 - 8j) = (0 + 5j) + (17 + 29j)
    assert out[0].tolist() == [17, 34] and clipped == 0
    assert out.tolist() == ar.combine_scalar([x0, x1], w, 0, 2)[0].tolist()
    out1, c1 = ar.combine_ref([x0, x1], w, 2, 1)                       # round half up: (17 + 2) >> 2 = 4, (34 + 2) >> 2 = 9
    assert out1[0].tolist() == [4, 9] and (out1.tolist(), c1) == (ar.combine_scalar([x0, x1], w, 2, 1)[0].tolist(), 0)
    big, cb = ar.combine_ref([x0 * 100, x1 * 100], w, 0, 1)            # every element past 127: all six clamped
    assert cb == 6 and np.abs(big).max() == 127
    assert (big.tolist(), cb) == (ar.combine_scalar([x0 * 100, x1 * 100], w, 0, 1)[0].tolist(), 6)


@pytest.mark.parametrize("in_size", [1, 2])
def test_power_of_the_combined_stream_is_the_quadratic_form_exactly(in_size):
    """shift 0, nothing clamped, int16 output: sum |y|^2 == sum_{a,b} w_a conj(w_b) R[a][b] in Python integers."""
    rng = np.random.default_rng(5 + in_size)
    nelem = 4
    xs = ar.streams(rng, nelem, 200, in_size)
    lim = 30                                                         # int8: |y| <= 4 * 2 * 30 * 128 = 30720, inside int16
    if in_size == 2:
        xs = [(x // 64).astype(np.int16) for x in xs]                  # int16: |x| <= 512 and |w| <= 7: |y| <= 4 * 2 * 7 * 512 = 28672
        lim = 7
    w = rng.integers(-lim, lim + 1, size=(nelem, 2))
    y, clipped = ar.combine_ref(xs, w, 0, 2)
    assert clipped == 0
    power = sum(int(v) * int(v) for v in y.ravel())
    re, im = ar.quadratic_form(w, ar.cov_ref(xs))
    assert (re, im) == (power, 0)
    # and the covariance of the one combined stream is that power
    assert ar.cov_ref([y])[0, 0].tolist() == [power, 0]


@pytest.mark.parametrize("in_size,out_size", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_one_element_is_the_complex_filter_with_one_tap(in_size, out_size):
    rng = np.random.default_rng(3)
    x = ar.streams(rng, 1, 300, in_size, "extremes")[0]
    for w, shift in (([[32767, -32768]], 14), ([[-3, 2]], 0), ([[-32768, 32767]], 24), ([[0, 1]], 0)):
        a, ca = ar.combine_ref([x], w, shift, out_size)
        b, cb = cr.cfilter_ref(x, None, w, shift, 1, 0, out_size)
        assert np.array_equal(a, b) and ca == cb


def test_steer_against_the_formula():
    for az, el in ((0.0, 0.0), (0.7, 0.3), (-2.1, 1.2), (3.0, -0.4), (np.pi / 2, 0.0)):
        got = gpsiq.array_steer(ar.SQUARE, az, el)
        want = ar.steer_ref(ar.SQUARE, az, el)
        d = np.abs(got - want)
        assert np.minimum(d, 1.0 - d).max() < 1e-14 and (got >= 0).all() and (got < 1).all()
    # due east along the ground: half a wavelength east is half a cycle, north is none
    assert np.allclose(gpsiq.array_steer(ar.SQUARE, np.pi / 2, 0.0), [0.0, 0.5, 0.0, 0.5], atol=1e-15)
    far = gpsiq.array_steer([[1000.25, -3.5, 2.0]], 0.0, 0.0)           # only north counts from due north: frac(-3.5) = 0.5
    assert abs(far[0] - 0.5) < 1e-12


def _v(w, shift):
    """the v of the contract from the integer weights: w = 2^shift conj(v)"""
    return (w[:, 0] - 1j * w[:, 1]) / float(1 << shift)


CASES = {
    "one jammer": (4, 1.0, [(1000.0, [0.0, 0.31, 0.77, 0.12])]),
    "two jammers": (4, 1.0, [(1000.0, [0.0, 0.31, 0.77, 0.12]), (300.0, [0.0, 0.9, 0.45, 0.6])]),
    "eight elements": (8, 2.0, [(5000.0, [0.0, 0.1, 0.25, 0.4, 0.55, 0.7, 0.85, 0.95])]),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("steered", [False, True], ids=["power inversion", "steered"])
def test_weights_solve_the_system(name, steered):
    """(a) With a large shift the rounded weights ARE v to within rounding, and v is held to numpy.linalg.solve in double.
    Tolerance: solve's relative error is about cond(Rn) * 2^-52 (backward stable LU), the library's long double Cholesky is smaller
    still, and rounding to integers adds at most 0.7072 / 2^shift per entry in absolute terms.  The covariances here have
    cond(Rn) = (sigma^2 + E J) / sigma^2 <= 2.1e4 (plus the second jammer's), so 1e-9 relative on |v| is three orders above the
    first term, and the second is added on its own.  The second term is the one that binds: the call hands out rounded integers only,
    and w_0 = 2^shift must fit int16, so through this entry point the solution is seen to about 0.7072 / 2^13 = 8.6e-5 and no finer;
    an error of the solver between 1e-9 and that would pass here.  test_weights_land_on_the_right_side_of_a_rounding_seam below looks
    closer."""
    nelem, sigma2, jam = CASES[name]
    nsamp = 1 << 20
    cov, rn = ar.model_cov(nelem, sigma2, jam, nsamp, scale=1 << 20)     # scaled so that rounding the model to integers is far below sigma^2
    steer = np.array([0.0, 0.2, 0.63, 0.41, 0.05, 0.5, 0.9, 0.33])[:nelem] if steered else None
    c = np.exp(2j * np.pi * steer) if steered else np.eye(nelem)[0].astype(np.complex128)
    z = np.linalg.solve(rn, c)
    want = z / (c.conj() @ z)
    assert np.linalg.cond(rn) < 1e5
    shift = 13                                                       # (two jammers: sum |w| is 5.6 * 2^shift, past the bound at 14)
    w = gpsiq.array_weights(cov, nsamp, steer=steer, loading=0.0, shift=shift).astype(np.int64)
    got = _v(w, shift)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max() + 0.7072 / (1 << shift)
    # (b) the constraint, in units of the integer weights: sum w_e c_e = 2^shift (v^H c) = 2^shift up to nelem / sqrt 2
    wc = ((w[:, 0] + 1j * w[:, 1]) * c).sum()
    assert abs(wc - (1 << shift)) <= nelem / np.sqrt(2.0) + 1e-6


@pytest.mark.parametrize("rotated", [False, True], ids=["real", "imaginary"])
def test_weights_land_on_the_right_side_of_a_rounding_seam(rotated):
    """Closer than rounding lets test_weights_solve_the_system look.  For two elements and c = e_0, v_1 = -R[1][0] / R[1][1] exactly.
    With R[0][0] = R[1][1] = P = 2^14 M and |R[1][0]| = Q = (2 k + 1) M -+ 1, 2^13 |v_1| = k + 1/2 -+ 1 / (2 M): half a unit either side
    of a rounding seam by 1 / (2 M) = 2^-31 of a unit, 1.2e-13 of the value at k = 2000.  The rounded weight must be k below the seam and
    k + 1 above it, so an error of the solver above about 1e-13 relative turns one of the two; cond(Rn) = (P + Q) / (P - Q) < 1.7, so
    neither long double nor double arithmetic is anywhere near that."""
    k, m, shift = 2000, 1 << 30, 13
    p = (1 << 14) * m
    for side, want in ((-1, k), (1, k + 1)):
        q = (2 * k + 1) * m + side
        cov = np.zeros((2, 2, 2), np.int64)
        cov[0, 0, 0] = cov[1, 1, 0] = p
        if rotated:                                                  # R[1][0] = j Q: v_1 = -j Q / P, w_1 = conj(v_1) 2^shift = +j ...
            cov[1, 0, 1], cov[0, 1, 1] = q, -q
        else:
            cov[1, 0, 0] = cov[0, 1, 0] = q
        w = gpsiq.array_weights(cov, 1, shift=shift).astype(np.int64)
        assert w.tolist() == [[1 << shift, 0], [0, want] if rotated else [-want, 0]], (side, w.tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_power_inversion_nulls_the_jammer(name):
    """(c) For Rn = s^2 I + J a a^H with |a_e| = 1 (a^H a = E) and c = e_0, the rank-one inverse is
      Rn^-1 = (I - J a a^H / D) / s^2,   D = s^2 + E J,
    so Rn^-1 e_0 = (e_0 - J conj(a_0) a / D) / s^2,  e_0^H Rn^-1 e_0 = (D - J) / (s^2 D),  v = (D e_0 - J conj(a_0) a) / (D - J) and
      a^H v = conj(a_0) (D - E J) / (D - J),   |v^H a| = s^2 / (s^2 + (E - 1) J).
    The residual jammer power J |v^H a|^2 = J s^4 / (s^2 + (E - 1) J)^2 is below s^2 for every E >= 2, because
    (s^2 + (E - 1) J)^2 >= (s^2 + J)^2 > J s^2.  The output power v^H Rn v = 1 / (e_0^H Rn^-1 e_0) <= Rn[0][0] because e_0 itself
    meets the constraint.  With two jammers the same two inequalities are checked on the model's own Rn.  The integer weights add
    rounding: each entry of v moves by at most 0.7072 / 2^shift, so |v^H a| moves by at most E * 0.7072 / 2^shift (`slack`)."""
    nelem, sigma2, jam = CASES[name]
    nsamp, shift = 1 << 20, 13
    cov, rn = ar.model_cov(nelem, sigma2, jam, nsamp, scale=1 << 20)
    w = gpsiq.array_weights(cov, nsamp, steer=None, loading=0.0, shift=shift).astype(np.int64)
    v = _v(w, shift)
    out_power = (v.conj() @ rn @ v).real
    slack = nelem * 0.7072 / (1 << shift)
    assert out_power <= rn[0, 0].real * (1 + 4 * slack)
    for power, cycles in jam:
        a = np.exp(2j * np.pi * np.asarray(cycles))
        assert power * (abs(v.conj() @ a) + slack) ** 2 < sigma2, name
        if len(jam) == 1:
            closed = sigma2 / (sigma2 + (nelem - 1) * power)
            assert abs(abs(v.conj() @ a) - closed) <= slack + 1e-9


def test_loading_fills_the_null_and_keeps_the_constraint():
    nelem, sigma2, jam = CASES["one jammer"]
    nsamp = 1 << 20
    cov, rn = ar.model_cov(nelem, sigma2, jam, nsamp, scale=1 << 20)
    a = np.exp(2j * np.pi * np.asarray(jam[0][1]))
    resid = []
    for loading in (0.0, 0.01, 1.0):
        w = gpsiq.array_weights(cov, nsamp, loading=loading, shift=14).astype(np.int64)
        assert abs(w[0, 0] - (1 << 14)) <= 1 and abs(w[0, 1]) <= 1     # c = e_0: w_0 = 2^shift
        resid.append(abs(_v(w, 14).conj() @ a))
    assert resid[0] < resid[1] < resid[2]


def test_refusals():
    cov, _ = ar.model_cov(4, 1.0, CASES["one jammer"][2], 1 << 20, scale=1 << 20)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.array_weights(cov, 0)
    E_ARG = e.value.code
    for kw in (dict(loading=-0.1), dict(loading=float("nan")), dict(loading=float("inf")), dict(shift=-1), dict(shift=25),
               dict(steer=[0.0, float("nan"), 0.0, 0.0])):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.array_weights(cov, 1 << 20, **kw)
        assert e.value.code == E_ARG, kw
    for bad in (np.zeros((4, 4, 2), np.int64), -cov):                 # singular, and negative definite
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.array_weights(bad, 1 << 20)
        assert e.value.code == E_ARG
    assert len(gpsiq.array_weights(np.zeros((4, 4, 2), np.int64) + np.eye(4, dtype=np.int64)[:, :, None] * [1, 0], 1, loading=0.5)) == 4
    # a weight that leaves int16: c = e_0 makes w_0 = 2^shift, out of range from shift 15 on
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.array_weights(cov, 1 << 20, shift=15)
    E_RANGE = e.value.code
    assert E_RANGE != E_ARG
    # the sum bound: a steered solution over eight equal elements has |w_e| = 2^shift / 8 in each of up to two components
    eye8 = np.zeros((8, 8, 2), np.int64)
    eye8[np.arange(8), np.arange(8), 0] = 1000
    st = np.full(8, 0.125)                                           # every weight on the diagonal re = im: 16 components
    assert np.abs(gpsiq.array_weights(eye8, 1000, steer=st, shift=14).astype(np.int64)).sum() <= 65535     # 16 * 1448 = 23168
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.array_weights(eye8, 1000, steer=st, shift=16)           # 16 * 5793 = 92688 > 65535, every entry inside int16
    assert e.value.code == E_RANGE
    for call in (lambda: gpsiq.array_steer(np.zeros((9, 3)), 0.0, 0.0), lambda: gpsiq.array_steer(ar.SQUARE, float("nan"), 0.0),
                 lambda: gpsiq.array_steer(ar.SQUARE, 0.0, float("inf")), lambda: gpsiq.array_steer(np.zeros((0, 3)), 0.0, 0.0)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call()
        assert e.value.code == E_ARG
    with pytest.raises(gpsiq.GpsiqError):
        gpsiq.array_weights(np.zeros((9, 9, 2), np.int64), 10)


def test_array_element_advances_the_carrier_phase_only():
    desc = np.zeros((3, 2), dtype=gpsiq.CHAN_DTYPE)
    desc["prn"] = [[1, 7]] * 3
    desc["carr_phase"] = [[0.25, 0.9], [0.5, 0.1], [0.75, 0.0]]
    desc["f_carr"] = 1234.5
    el = gpsiq.array_element(desc, [0.5, 0.2])
    assert np.allclose(el["carr_phase"], [[0.75, 0.1], [0.0, 0.3], [0.25, 0.2]], atol=1e-15)
    assert (el["carr_phase"] >= 0).all() and (el["carr_phase"] < 1).all()
    for name in desc.dtype.names:
        if name != "carr_phase":
            assert np.array_equal(el[name], desc[name])
    assert desc["carr_phase"][0, 0] == 0.25                            # the argument stays as it is
    with pytest.raises(gpsiq.GpsiqError):
        gpsiq.array_element(desc, [0.5])
