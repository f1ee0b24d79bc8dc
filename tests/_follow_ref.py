"""numpy restatement of gpsiq_follow's contract (include/gpsiq_rows.h, "Follow"), written from the header and not from the kernel.
follow() is vectorised per epoch: the samples of an epoch are numpy arrays (64-bit wrapping arithmetic where the contract reduces mod
2^59, a split of the code step where n * c leaves 64 bits), the loop itself Python integers.  follow_scalar() is the same text once
more as a sample-by-sample loop of Python integers that shares nothing with follow() but the tables; tests/test_follow_ref.py holds
the two against each other.  Also the host helpers' formulas (gains, bits), the truth of a rendered channel for the signal tests, and the GPU case table made
real.  TEST INFRASTRUCTURE."""
import numpy as np

from gpsiq.abi import FOLLOW_CFG_DTYPE, FOLLOW_EPOCH_DTYPE, FOLLOW_STATE_DTYPE

PERIOD = 1023 << 56
MASK56, MASK59 = (1 << 56) - 1, (1 << 59) - 1
RUNNING, SPAN_END, FULL, RANGE = 0, 1, 2, 3
SUMS = ("ie", "qe", "ip", "qp", "il", "ql")
_U = np.uint64


def cdiv(a, b):
    """C's division of int64_t: toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def make_cfg(spacing=1 << 55, pull_epochs=100, kf=0, kp=0, ki=0, kd=0):
    c = np.zeros(1, dtype=FOLLOW_CFG_DTYPE)
    c["spacing"], c["pull_epochs"], c["kf"], c["kp"], c["ki"], c["kd"] = spacing, pull_epochs, kf, kp, ki, kd
    return c


def make_state(prn, sample=0, chip=0, code_frac=0, code_step0=None, code_step=None, carr_phase=0, carr_step=0, carr_int=None, prev=None, epoch=0):
    s = np.zeros(1, dtype=FOLLOW_STATE_DTYPE)
    step0 = code_step if code_step0 is None else code_step0
    s["prn"], s["sample"], s["chip"], s["code_frac"], s["code_step0"], s["code_step"] = prn, sample, chip, code_frac, step0, step0 if code_step is None else code_step
    s["carr_phase"], s["carr_step"], s["carr_int"], s["epoch"] = carr_phase, carr_step, carr_step if carr_int is None else carr_int, epoch
    if prev is not None:
        s["prev_ip"], s["prev_qp"], s["have_prev"] = prev[0], prev[1], 1
    return s[0]


def in_range(code_step, carr_step):
    return (1 << 52) <= code_step < (1 << 57) and abs(carr_step) < (1 << 58)


def _tap_chips(base, c, n):
    """int64 [len(n)]: ((base + n * c) >> 56) mod 1023 for base < 2^67, c < 2^57, n < 2^14 (uint64): n * c is taken in two halves of
    28 bits so that nothing leaves 64 bits"""
    hi, lo = base >> 56, base & MASK56
    a = n * _U(c >> 28) + _U(lo >> 28)                                   # units of 2^28: below 2^44
    b = n * _U(c & ((1 << 28) - 1)) + _U(lo & ((1 << 28) - 1))           # units of 1: below 2^43
    whole = (a + (b >> _U(28))) >> _U(28)                                # floor((lo + n * c) / 2^56), exactly
    return ((_U(hi) + whole) % _U(1023)).astype(np.int64)


def _close(s, cfg, N, X):
    """steps 5 to 10 on a state dict of Python integers"""
    top = max(abs(v) for v in X)
    sh = max(0, top.bit_length() - 22)
    ie, qe, ip, qp, il, ql = (v >> sh for v in X)
    num, den = (ie - il) * ip + (qe - ql) * qp, ip * ip + qp * qp
    ed = cdiv(num << 16, den) if den else 0
    ed = max(-(1 << 16), min(1 << 16, ed))
    if s["epoch"] < cfg["pull_epochs"]:
        if s["have_prev"]:
            cross, dot = s["prev_ip"] * qp - s["prev_qp"] * ip, s["prev_ip"] * ip + s["prev_qp"] * qp
            if dot < 0:
                cross = -cross
            d = abs(cross) + abs(dot)
            ef = cdiv(cross << 16, d) if d else 0
            s["carr_int"] += (ef * cfg["kf"]) >> 16
        w = s["carr_int"]
    else:
        numc, denc = (qp if ip >= 0 else -qp), abs(ip) + abs(qp)
        ec = cdiv(numc << 16, denc) if denc else 0
        s["carr_int"] += (ec * cfg["ki"]) >> 16
        w = s["carr_int"] + ((ec * cfg["kp"]) >> 16)
    s["carr_phase"] = (s["carr_phase"] + N * s["carr_step"]) % (1 << 59)
    total = s["code_frac"] + N * s["code_step"]
    s["chip"], s["code_frac"] = s["chip"] + (total >> 56) - 1023, total & MASK56
    s["sample"] += N
    s["prev_ip"], s["prev_qp"], s["have_prev"] = ip, qp, 1
    s["epoch"] += 1
    s["carr_step"] = w
    s["code_step"] = s["code_step0"] + cdiv(w, 12320) + ((ed * cfg["kd"]) >> 16)


_INT_FIELDS = [f for f in FOLLOW_STATE_DTYPE.names if f != "reserved"]


def _unpack(state):
    return {f: int(state[f]) for f in _INT_FIELDS}


def _pack(s):
    out = np.zeros(1, dtype=FOLLOW_STATE_DTYPE)
    for f in _INT_FIELDS:
        out[f] = s[f] % (1 << 64) if f == "code_step" else s[f]          # (a code step that left its range is stored in 64 bits as it is)
    return out[0]


def follow(orc, stream, cfg, states, max_epochs):
    """stream: integer array of interleaved I, Q (the whole span); cfg: FOLLOW_CFG_DTYPE element; states: FOLLOW_STATE_DTYPE [nprn] ->
    (records FOLLOW_EPOCH_DTYPE [nprn][max_epochs], nepochs int32 [nprn], states FOLLOW_STATE_DTYPE [nprn])"""
    sn, cs = (t.astype(np.int64) for t in orc.tables())
    x = np.asarray(stream).astype(np.int64).reshape(-1, 2)
    nsamp = len(x)
    cfg = {f: int(np.asarray(cfg).ravel()[0][f]) for f in FOLLOW_CFG_DTYPE.names}
    states = np.atleast_1d(np.asarray(states, dtype=FOLLOW_STATE_DTYPE))
    rec = np.zeros((len(states), max_epochs), dtype=FOLLOW_EPOCH_DTYPE)
    count = np.zeros(len(states), dtype=np.int32)
    out = np.zeros(len(states), dtype=FOLLOW_STATE_DTYPE)
    for p in range(len(states)):
        s = _unpack(states[p])
        if s["code_step"] >= 1 << 63:
            s["code_step"] -= 1 << 64
        sign = 1 - 2 * orc.codegen(s["prn"]).astype(np.int64)
        k = 0
        while True:
            if not in_range(s["code_step"], s["carr_step"]):
                s["status"] = RANGE
                break
            T0, c, w, m = (s["chip"] << 56) + s["code_frac"], s["code_step"], s["carr_step"], s["sample"]
            N = -((T0 - PERIOD) // c)
            if m + N > nsamp:
                s["status"] = SPAN_END
                break
            if k == max_epochs:
                s["status"] = FULL
                break
            n = np.arange(N, dtype=np.uint64)
            idx = (((_U(s["carr_phase"]) + n * _U(w % (1 << 64))) & _U(MASK59)) >> _U(50)).astype(np.int64)
            xi, xq = x[m:m + N, 0], x[m:m + N, 1]
            yi, yq = xi * cs[idx] + xq * sn[idx], xq * cs[idx] - xi * sn[idx]
            X = []
            for off in (cfg["spacing"], 0, -cfg["spacing"]):
                base = T0 + off
                if base < 0:
                    base += PERIOD
                ca = sign[_tap_chips(base, c, n)]
                X += [int((yi * ca).sum()), int((yq * ca).sum())]
            r = rec[p, k]
            r["sample"], r["nsamp"], r["chip"], r["code_frac"], r["code_step"], r["carr_phase"], r["carr_step"] = m, N, s["chip"], s["code_frac"], c, s["carr_phase"], w
            for f, v in zip(SUMS, X):
                r[f] = v
            k += 1
            _close(s, cfg, N, X)
        count[p] = k
        out[p] = _pack(s)
    return rec, count, out


def follow_rebased(orc, tail, base, cfg, states, max_epochs):
    """follow() on a span too long to hold, from its tail: `tail` the elements of samples [base, nsamp) of the span, every state's
    `sample` at or past base.  Nothing in an epoch depends on the absolute sample but where it reads (the carrier runs from carr_phase),
    so the run is follow() on the tail with `sample` rebased in the states going in, and in the records and states coming out."""
    states = np.array(np.atleast_1d(states), dtype=FOLLOW_STATE_DTYPE, copy=True)
    assert all(int(s) >= base for s in states["sample"])
    states["sample"] -= np.uint64(base)
    rec, count, out = follow(orc, tail, cfg, states, max_epochs)
    for p in range(len(states)):
        rec["sample"][p, :count[p]] += np.uint64(base)
    out["sample"] += np.uint64(base)
    return rec, count, out


def follow_scalar(orc, stream, cfg, state, max_epochs):
    """one satellite, the contract sample by sample in Python integers -> (list of record tuples in FOLLOW_EPOCH_DTYPE's field order
    without `reserved`, final state as a dict)"""
    sin_t, cos_t = orc.tables()
    code = [int(v) for v in orc.codegen(int(state["prn"]))]
    flat = [int(v) for v in np.asarray(stream).ravel()]
    total_samples = len(flat) // 2
    g = lambda f: int(np.asarray(cfg).ravel()[0][f])
    spacing, pull, kf, kp, ki, kd = g("spacing"), g("pull_epochs"), g("kf"), g("kp"), g("ki"), g("kd")
    st = {f: int(state[f]) for f in FOLLOW_STATE_DTYPE.names if f != "reserved"}
    trunc = lambda a, b: int(abs(a) // abs(b)) * (1 if (a >= 0) == (b > 0) else -1)
    records = []
    while True:
        c, w = st["code_step"], st["carr_step"]
        if c < 2 ** 52 or c >= 2 ** 57 or w <= -2 ** 58 or w >= 2 ** 58:
            st["status"] = 3
            break
        T0 = st["chip"] * 2 ** 56 + st["code_frac"]
        N = (1023 * 2 ** 56 - T0 + c - 1) // c
        if st["sample"] + N > total_samples:
            st["status"] = 1
            break
        if len(records) == max_epochs:
            st["status"] = 2
            break
        sums = [0] * 6
        for n in range(N):
            idx = ((st["carr_phase"] + n * w) % 2 ** 59) >> 50
            i, q = flat[2 * (st["sample"] + n)], flat[2 * (st["sample"] + n) + 1]
            yi, yq = i * int(cos_t[idx]) + q * int(sin_t[idx]), q * int(cos_t[idx]) - i * int(sin_t[idx])
            for t, off in enumerate((spacing, 0, -spacing)):
                A = T0 + off + n * c
                if T0 + off < 0:
                    A += 1023 * 2 ** 56
                ca = -1 if code[(A >> 56) % 1023] else 1
                sums[2 * t] += yi * ca
                sums[2 * t + 1] += yq * ca
        records.append((st["sample"], st["code_frac"], c, st["carr_phase"], w) + tuple(sums) + (N, st["chip"]))
        big = max(abs(v) for v in sums)
        sh = max(0, big.bit_length() - 22)
        ie, qe, ip, qp, il, ql = [v >> sh for v in sums]
        den = ip * ip + qp * qp
        ed = trunc(((ie - il) * ip + (qe - ql) * qp) * 65536, den) if den else 0
        ed = -65536 if ed < -65536 else 65536 if ed > 65536 else ed
        if st["epoch"] < pull:
            if st["have_prev"]:
                cross = st["prev_ip"] * qp - st["prev_qp"] * ip
                dot = st["prev_ip"] * ip + st["prev_qp"] * qp
                cross = -cross if dot < 0 else cross
                ef = trunc(cross * 65536, abs(cross) + abs(dot)) if abs(cross) + abs(dot) else 0
                st["carr_int"] += (ef * kf) >> 16
            w_next = st["carr_int"]
        else:
            numc = qp if ip >= 0 else -qp
            ec = trunc(numc * 65536, abs(ip) + abs(qp)) if abs(ip) + abs(qp) else 0
            st["carr_int"] += (ec * ki) >> 16
            w_next = st["carr_int"] + ((ec * kp) >> 16)
        st["carr_phase"] = (st["carr_phase"] + N * w) % 2 ** 59
        adv = st["code_frac"] + N * c
        st["chip"] += (adv >> 56) - 1023
        st["code_frac"] = adv % 2 ** 56
        st["sample"] += N
        st["prev_ip"], st["prev_qp"], st["have_prev"] = ip, qp, 1
        st["epoch"] += 1
        st["carr_step"] = w_next
        st["code_step"] = st["code_step0"] + trunc(w_next, 12320) + ((ed * kd) >> 16)
    return records, st


RECORD_FIELDS = ("sample", "code_frac", "code_step", "carr_phase", "carr_step") + SUMS + ("nsamp", "chip")


def record_tuple(r):
    return tuple(int(r[f]) for f in RECORD_FIELDS)


# ---- the host helpers -------------------------------------------------------------------------------------------------------------------
def gains(fs, fll_gain, pll_bn_hz, dll_bn_hz):
    """gpsiq_follow_gains' formulas -> dict"""
    n0, wn = fs / 1000.0, pll_bn_hz / 0.53
    return dict(spacing=1 << 55, pull_epochs=100,
                kf=int(np.rint(fll_gain * 2.0 ** 59 / (2.0 * np.pi * n0))), ki=int(np.rint(wn * wn * 1e-3 / (2.0 * np.pi) * 2.0 ** 59 / fs)),
                kp=int(np.rint(1.414 * wn / (2.0 * np.pi) * 2.0 ** 59 / fs)), kd=int(np.rint(4.0 * dll_bn_hz / (2.0 * fs) * 2.0 ** 56)))


def bits(ip, skip):
    """gpsiq_follow_bits' rule on the in-phase prompts of one satellite: (offset, int8 bits), or None where the library answers
    GPSIQ_E_RANGE"""
    v = np.asarray(ip, dtype=np.int64)[skip:]
    if len(v) < 40:
        return None
    groups = lambda o: v[o:o + 20 * ((len(v) - o) // 20)].reshape(-1, 20).sum(axis=1)
    metric = [int(np.abs(groups(o)).sum()) for o in range(20)]
    o = int(np.argmax(metric))                                            # the first of equals
    return o, np.sign(groups(o)).astype(np.int8)


# ---- truth of a rendered channel, from its quantised descriptors (include/gpsiq.h's closed form) ----------------------------------------
def truth_code_phase(qc, n):
    """code phase in chips (float, exact to 2^-53 relative) of quantised descriptor qc at sample n of its block"""
    T = int(qc["code_frac"]) + n * int(qc["code_step"])
    return ((int(qc["chip0"]) + (T >> 56)) % 1023) + (T & MASK56) / 2.0 ** 56


def truth_data_bit(qc, n):
    """the data bit (0 / 1) under sample n of the block"""
    T = int(qc["code_frac"]) + n * int(qc["code_step"])
    A = int(qc["chip0"]) + (T >> 56)
    return (int(qc["nav_bits"]) >> ((int(qc["icode"]) + A // 1023) // 20)) & 1


# ---- a case of tests/_follow_plan.py's table made real ----------------------------------------------------------------------------------
def case_stream(case, index):
    """the elements of the case's span (before any cut): seeded by the case's place in the table"""
    from gpsiq.abi import elem_dtype
    dt = elem_dtype(case.ss)
    info = np.iinfo(dt)
    if case.stream != "random":
        return np.full(2 * case.nsamp, dict(min=info.min, max=info.max, zero=0)[case.stream], dtype=dt)
    x = np.random.default_rng(9000 + index).integers(info.min, info.max + 1, size=2 * case.nsamp).astype(dt)
    x[:2], x[-2:] = info.min, info.max                                    # the extremes at either end of the span
    return x


def materialise(orc, case, index):
    """-> (stream, cfg, states, (records, nepochs, states out)) of a case; a case with a cut has its span shortened to end on the last
    sample of the named record, and the reference taken again on the shortened span"""
    stream, cfg = case_stream(case, index), make_cfg(**case.cfg)
    states = np.array([make_state(**s) for s in case.states], dtype=FOLLOW_STATE_DTYPE)
    ref = follow(orc, stream, cfg, states, case.max_epochs)
    if case.cut is not None:
        p, k = case.cut
        assert ref[1][p] > k
        end = int(ref[0][p, k]["sample"]) + int(ref[0][p, k]["nsamp"])
        stream = stream[:2 * end].copy()
        ref = follow(orc, stream, cfg, states, case.max_epochs)
        assert ref[1][p] == k + 1 and int(ref[2][p]["sample"]) == end and ref[2][p]["status"] == SPAN_END
    return stream, cfg, states, ref
