"""The output level stage behind the list-overflow fall-back of the device-evaluated batch: the one path where a call is rendered
a second time, on the host-evaluated route with patches, noise and level, after the device route has already written the
destination.  No honest input overflows the lists, so this needs the library built with -DGPSIQ_TEST_HOOKS (never the shipped
build), which shortens them on request (GPSIQ_TEST_LIST_CAP); built here the way tests/test_gpu_verify.py builds it, used from a
child process.  GPSIQ_NCO_REFERENCE at 25 Msps, where every block has patches; every element compared with tests/_level_ref.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpsiq
import _level_ref as lr
import _noise_ref as nr
from gpsiq.abi import NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks
assert os.path.samefile(gpsiq.LIB_PATH, os.environ["GPSIQ_LIB"])
assert os.path.samefile(os.path.dirname(gpsiq.ROWS_PATH), os.path.dirname(gpsiq.LIB_PATH))
fs, ns, nb, nc = 25e6, 2500000, 50, 8
seed, sigma, base, qmax = 0xFA11, 4970.0, 300, 127
mult = gpsiq.level_mult(sigma, qmax / 3.0)
d = synth_blocks(nb, nc, seed=45)
ctx = gpsiq.Context(0)
ctx.set_nco_mode(NCO_REFERENCE)
os.environ["GPSIQ_EVAL"] = "host"
clean = ctx.generate_batch(d, ns, fs, SC16)                                 # level and noise off: the restatement's S
ctx.set_noise(seed, sigma, base)
ctx.set_level(mult, qmax)
carr_h = np.zeros(nc)
want = ctx.generate_batch(d, ns, fs, SC08, carr_out=carr_h)
for b0 in range(0, nb, 10):                                                 # the host-evaluated render is the restatement's
    z = nr.noise(seed, sigma, base + b0, 10, ns)
    assert np.array_equal(want[b0:b0 + 10], lr.level(clean[b0:b0 + 10], z, mult, qmax, 1)), b0
del clean
os.environ["GPSIQ_EVAL"] = "device"
ctx.set_noise(seed, sigma, base)
s0 = gpsiq.device_eval_stats()
carr_d = np.zeros(nc)
got = ctx.generate_batch(d, ns, fs, SC08, carr_out=carr_d)
s1 = gpsiq.device_eval_stats()
assert s1[0] == s0[0] + 1 and s1[4] - s0[4] > 8 and s1[5] == s0[5], (s0, s1)   # device path, patches there are, the lists held them
assert np.array_equal(got, want) and carr_d.tobytes() == carr_h.tobytes()
os.environ["GPSIQ_TEST_LIST_CAP"] = "3"
ctx.set_noise(seed, sigma, base)
carr_f = np.zeros(nc)
got = ctx.generate_batch(d, ns, fs, SC08, carr_out=carr_f)
s2 = gpsiq.device_eval_stats()
assert s2[5] == s1[5] + 1, (s1, s2)                                         # fell back: rendered again on the host-evaluated route
assert np.array_equal(got, want) and carr_f.tobytes() == carr_h.tobytes()
assert ctx.noise_state() == (seed, sigma, base + nb), ctx.noise_state()     # numbered once, not once per render
del os.environ["GPSIQ_TEST_LIST_CAP"]
ctx.set_noise(seed, sigma, base)
got = ctx.generate_batch(d, ns, fs, SC08)                                   # and the context is as good as before
assert np.array_equal(got, want) and gpsiq.device_eval_stats()[5] == s2[5]
ctx.close()
print("all ok")
'''


@pytest.mark.gpu
def test_fall_back_renders_noise_and_level_like_the_host_route(tmp_path):
    out = str(tmp_path / "libgpsiq_hooks.so")
    b = subprocess.run(["make", "-B", "-s", "-C", os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc"), "OUT=" + out, "EXTRA=-DGPSIQ_TEST_HOOKS"],
                       capture_output=True, text=True, timeout=900)
    assert b.returncode == 0 and os.path.getsize(out) > 100000, b.stderr[-3000:]
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], env=dict(os.environ, GPSIQ_LIB=out), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
