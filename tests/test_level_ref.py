"""The output level stage (include/gpsiq_rows.h, "Output level") without a GPU: the helpers against their formulas, where the calls
are exported, and the reason the stage exists -- a stream with a realistic noise floor saturates a fraction of a percent of its
samples instead of wrapping a fifth or more of them -- on the numpy restatement (tests/_level_ref.py)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import _level_ref as lr
import _noise_ref as nr
import gpsiq
from gpsiq.abi import SC16

# (fs, C/N0): the configurations whose int8 stream wraps today; sigma is what gpsiq_runahead --cn0 sets
ROWS = [(2.6e6, 45.0), (2.6e6, 40.0), (10e6, 45.0), (25e6, 45.0), (25e6, 35.0)]


def test_helpers_match_their_formulas():
    rng = np.random.default_rng(1)
    for _ in range(50):
        g = rng.uniform(-3.0, 3.0, rng.integers(0, 17))
        sigma = float(rng.uniform(0.0, 20000.0))
        want = math.sqrt(sigma * sigma + float(np.sum((250.0 * g) ** 2 / 2.0)))
        assert gpsiq.composite_rms(g, sigma) == pytest.approx(want, rel=1e-14)
        assert lr.composite_rms(g, sigma) == pytest.approx(want, rel=1e-14)
        rin, rout = float(rng.uniform(1.0, 30000.0)), float(rng.uniform(0.3, 11000.0))
        assert gpsiq.level_mult(rin, rout) == int(np.rint(65536.0 * rout / rin)) == lr.level_mult(rin, rout)
    assert gpsiq.composite_rms([], 0.0) == 0.0 and gpsiq.composite_rms([1.0], 0.0) == pytest.approx(250.0 / math.sqrt(2.0))


def test_level_mult_is_clamped_to_the_valid_range():
    assert gpsiq.level_mult(1e9, 1.0) == 1                      # rounds to 0
    assert gpsiq.level_mult(1.0, 1e9) == 2 ** 24 - 1
    assert gpsiq.level_mult(1.0, 255.99999) == 2 ** 24 - 1     # rint gives 2^24: one past the range
    assert gpsiq.level_mult(0.0, 1.0) == 2 ** 24 - 1 and gpsiq.level_mult(0.0, 0.0) == 1 and gpsiq.level_mult(1.0, -1.0) == 1
    assert gpsiq.level_mult(65536.0, 1.0) == 1 and gpsiq.level_mult(2.0, 1.0) == 32768


def test_set_level_is_exported_by_the_rows_library_only():
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {l.split()[2] for l in out.splitlines() if " T gpsiq_" in l}
    rows, core = exported(gpsiq.ROWS_PATH), exported(gpsiq.LIB_PATH)
    for name in ("gpsiq_set_level", "gpsiq_composite_rms", "gpsiq_level_mult"):
        assert name in rows and name not in core, name
    # the implementation is in the boundary library, behind its plumbing entry
    lib = C.CDLL(gpsiq.LIB_PATH)
    lib.gpsiq_plumbing.restype = C.c_void_p
    lib.gpsiq_plumbing.argtypes = [C.c_char_p]
    assert lib.gpsiq_plumbing(b"set_level")
    assert C.sizeof(gpsiq.LevelSettings) == 8


def test_a_null_context_is_refused():
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._set_level(None, None))
    assert e.value.code == -1


@pytest.mark.parametrize("qmax", [127, 32767])
@pytest.mark.parametrize("fs,cn0", ROWS)
def test_noise_floor_saturates_and_never_wraps(fs, cn0, qmax):
    """Pure noise at the sigma of each configuration, levelled to an rms of a third of full scale: every output is inside
    [-qmax, qmax], and the share that sits on the clamp is the share of the 65 536 equally likely table values that does."""
    sigma = gpsiq.noise_sigma_for_cn0(cn0, 1.0, fs)
    mult = gpsiq.level_mult(sigma, qmax / 3.0)
    assert 1 <= mult < 2 ** 24
    nb, ns = 8, 65536
    z = nr.noise(0xC0FFEE, sigma, 5, nb, ns)
    out = lr.stage(z, mult, qmax)
    assert out.min() >= -qmax and out.max() <= qmax
    p = float(np.mean(np.abs(lr.stage(lr.table_values(sigma), mult, qmax)) == qmax))       # exact
    n = out.size
    got = float(np.mean(np.abs(out) == qmax))
    se = math.sqrt(p * (1.0 - p) / n)
    print(f"fs {fs:g} cn0 {cn0:g} sigma {sigma:.0f} qmax {qmax}: saturated {got:.5f}, exact {p:.5f}, standard error {se:.2e}")
    assert 0.0 < p < 0.01 and abs(got - p) <= 5.0 * se
    # the rule it replaces: the same noise through today's int8 store lands on the wrong side of zero for a large share
    if qmax == 127:
        wrapped = np.mean(((z + 32768) % 65536 - 32768 >> 4 != z >> 4) | (np.abs(z >> 4) > 127))
        assert wrapped > 0.15


def test_unit_level_reproduces_the_int16_stream():
    """mult = 65536, qmax = 32767 is the identity wherever the sum is not -32768 (the clamp is symmetric)."""
    import _oracle
    from gpsiq.scenario import synth_blocks
    orc = _oracle.load_oracle()
    nsamp = 26000
    for gain in (1.0, 9.0):                                      # inside the int16 range, and wrapping sums
        desc = synth_blocks(2, 16, seed=3)
        desc["gain"] = gain
        q, _ = gpsiq.quantize_blocks(desc, 2.6e6, nsamp)
        for b in range(2):
            clean = orc.block_fixed(q[b], nsamp, SC16, seq=True)
            out = lr.level(clean[None], None, 65536, 32767, 2)[0]
            keep = clean != -32768
            assert np.array_equal(out[keep], clean[keep]) and np.all(out[~keep] == -32767)
