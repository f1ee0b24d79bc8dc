"""numpy restatement of gpsiq_despread's contract (include/gpsiq_rows.h, "Despread").  The replica of a channel is the oracle's
closed form (Oracle.block_fixed) of that one descriptor with gain 1.0 in int16; sums and stream statistics are then int64 numpy,
and device order is a block's active channels in input order.  Nothing else restates the closed form.  TEST INFRASTRUCTURE."""
import numpy as np

import _oracle
from gpsiq.abi import BLOCK_STATS_DTYPE, DESPREAD_SUM_DTYPE, QCHAN_DTYPE, SC16


def replica(orc, qc, nsamp):
    """int64 [nsamp, 2]: (rI, rQ) of one quantised descriptor"""
    one = np.zeros(1, dtype=QCHAN_DTYPE)
    one[0] = qc
    one["gain"] = 1.0
    return orc.block_fixed(one, nsamp, SC16).astype(np.int64).reshape(nsamp, 2)


def nseg_of(nsamp, seg_len):
    return -(-nsamp // seg_len)


def despread(orc, q, stream, nsamp, seg_len):
    """q: QCHAN_DTYPE [nblocks][nchan]; stream: integer array [nblocks][2 * nsamp] (interleaved I, Q as stored) ->
    (sums DESPREAD_SUM_DTYPE [nblocks][nchan][nseg], prn uint8 [nblocks][nchan])"""
    nb, nc = q.shape
    nseg = nseg_of(nsamp, seg_len)
    sums = np.zeros((nb, nc, nseg), dtype=DESPREAD_SUM_DTYPE)
    prn = np.zeros((nb, nc), dtype=np.uint8)
    starts = np.arange(0, nsamp, seg_len)
    for b in range(nb):
        x = np.asarray(stream[b]).astype(np.int64).reshape(nsamp, 2)
        k = 0
        for c in range(nc):
            if q[b, c]["prn"] == 0:
                continue
            r = replica(orc, q[b, c], nsamp)
            prn[b, k] = q[b, c]["prn"]
            if nsamp:
                sums["i"][b, k] = np.add.reduceat(x[:, 0] * r[:, 0] + x[:, 1] * r[:, 1], starts)
                sums["q"][b, k] = np.add.reduceat(x[:, 1] * r[:, 0] - x[:, 0] * r[:, 1], starts)
            k += 1
    return sums, prn


def stats(stream, nsamp, clip):
    """BLOCK_STATS_DTYPE [nblocks] of the stream's own elements"""
    st = np.zeros(len(stream), dtype=BLOCK_STATS_DTYPE)
    for b in range(len(stream)):
        x = np.asarray(stream[b]).astype(np.int64).reshape(nsamp, 2)
        for k, f in enumerate("iq"):
            st["sum_" + f][b] = x[:, k].sum()
            st["sumsq_" + f][b] = (x[:, k] * x[:, k]).sum()
            st["clip_" + f][b] = int((np.abs(x[:, k]) >= clip).sum())
    return st


def cn0_estimate(sums, seg_len, fs):
    """the estimator of include/gpsiq_rows.h in numpy: (cn0_dbhz, one_sigma_db)"""
    i, qq = sums["i"].astype(np.float64).ravel(), sums["q"].astype(np.float64).ravel()
    n, T = len(i), seg_len / fs
    m = i.mean()
    v = (((i - m) ** 2).sum() / (n - 1) + (qq ** 2).sum() / n) / 2.0
    cn0 = 10.0 * np.log10(m * m / (2.0 * v * T))
    return cn0, (10.0 / np.log(10.0)) * np.sqrt(1.0 / n + 1.0 / (n * T * 10.0 ** (cn0 / 10.0)))


# ---- the closed loop: one channel at a set C/N0 and one noise-floor probe (tests/test_despread_ref.py, tests/test_gpu_despread.py) ----
LOOP = dict(fs=2.6e6, nsamp=66560, nblocks=64, seg_len=2560, cn0=45.0, gain=2.0, seed=0xC0DE45, prn=(7, 19))


def loop_descriptors(with_probe=True):
    """CHAN_DTYPE [nblocks][2]: slot 0 the channel at gain 2, slot 1 a probe at gain 0 (another satellite), or unused"""
    from gpsiq.scenario import synth_blocks
    d = synth_blocks(LOOP["nblocks"], 2, seed=45)
    d["prn"][:, 0], d["prn"][:, 1] = LOOP["prn"][0], LOOP["prn"][1] if with_probe else 0
    d["gain"][:, 0], d["gain"][:, 1] = LOOP["gain"], 0.0
    return d
