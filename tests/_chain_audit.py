"""The audit of the carrier chain's certified maps (csrc/gpsiq_lane.h) over their WHOLE range, and the timelines that put events on
the edges of the chain kernels (csrc/gpsiq_chain_kernels.hip).  Helpers only: pure numpy plus host calls of the library, no GPU.
tests/test_chain_audit.py holds this module to itself and audits the host twin's maps; tests/test_gpu_chain_edges.py audits
the device's.

A map says: a start state xs + d U (U = 2^-53) with lo <= d <= hi, d a multiple of the wrap's grid and of a parity ok allows, ends
on e + (d + cum[parity]) U.  Every other test pushes the one true start state through it (d a handful of units near 0); here the
claim is tried at lo, at hi, either side of them, per parity and in between, against the reference's accumulator started there.

A timeline comes with a RECORD of what was put where: [{"kind": ..., "slot": ..., "block": ...}, ...], "block" the block the event
was meant for (test_chain_audit.py checks that it sits there)."""
import numpy as np

import gpsiq
from gpsiq.abi import CHAIN_IN_DTYPE, CHAIN_EST_DTYPE, CHAIN_EXACT, CHAIN_RESEEDED

# ---- thresholds and edges, restated from the source as it stands ------------------------------------------------------------------
K_PREP_THREADS = 1024       # gpsiq_chain_kernels.hip kPrepThreads: blocks of one slot per round of chain_prepare (waves of 64)
K_WAVE = 64                 # the width of the shuffles in block_scan
K_LANE_THREADS = 256        # gpsiq_chain_kernels.hip kLaneThreads: a workgroup of chain_lanes<kSeg> holds 256 / kSeg blocks of a slot
K_TAB_MIN_SEG = 16          # gpsiq_chain_kernels.hip kTabMinSeg: chain_lanes<16> and <32> build a block's table of cycles
K_TAB = 22                  # gpsiq_lane.h lane::kTab: the lanes walk |c| >= 2^-22 ...
K_TOP = 6                   # gpsiq_walk.h FpWalk::setup_head (ec > 1022 - 6 is general): ... and |c| < 2^-6
K_ENTRIES_HOST = 32         # gpsiq_lane.h lane::kEntriesHost: a table when |c| nsamp > 2 kEntriesHost = 64
K_MAX_SEG = 32              # gpsiq_lane.h lane::kMaxSeg
C_MIN, C_MAX = 2.0 ** -K_TAB, 2.0 ** -K_TOP
WALK_MAX = 4096             # audit(): blocks up to here are held to walk(), longer ones to serial_end()
U = 2.0 ** -53
_K = 1074                   # every double is a whole number of 2^-1074
_SH = _K - 53
_ONE = 1 << _K


def stretches(c, nsamp, max_seg):
    """gpsiq_lane.h lane::stretches"""
    s = (np.abs(np.asarray(c, dtype=np.float64)) * float(nsamp) * 0.25).astype(np.int64)
    return np.clip(s, 1, max_seg)


def lanes_per_block(max_seg):
    """gpsiq_chain_kernels.hip launch_chain: the instantiation chain_lanes<kSeg> a launch takes"""
    return 32 if max_seg > 16 else 16 if max_seg > 8 else 8 if max_seg > 4 else 4


def walked_by_lanes(c):
    """FpWalk::setup_head: not `general`"""
    a = np.abs(np.asarray(c, dtype=np.float64))
    return (a >= C_MIN) & (a < C_MAX)


# ---- the references -------------------------------------------------------------------------------------------------------------
def walk(x, c, nsamp):
    """gps.c:2821-2826 over a vector of start states: per sample x += c; if (x >= 1.0) x -= 1.0; else if (x < 0.0) x += 1.0.
    c = f_carr * (1 / fs), computed once by the caller as the library does."""
    x = np.array(np.broadcast_to(np.asarray(x, dtype=np.float64), np.broadcast(x, c).shape), dtype=np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), x.shape)
    for _ in range(int(nsamp)):
        x = x + c
        over, under = x >= 1.0, x < 0.0
        x = np.where(over, x - 1.0, np.where(under, x + 1.0, x))
    return x


def serial_end(x, prn, f_carr, fs, nsamp):
    """The same through gpsiq.reference_chain, many probes per call: probe k is a pair of blocks in column k % 16, both of one
    satellite; the pair underneath it takes another satellite and so seeds itself from its own carr_phase.  The state after a
    pair's first block is carr_start of its second."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    n = x.size
    f = np.broadcast_to(np.asarray(f_carr, dtype=np.float64), x.shape)
    p = np.broadcast_to(np.asarray(prn, dtype=np.int32), x.shape)
    if n == 0:
        return np.zeros(0)
    cols = 16
    rows = -(-n // cols)
    cin = np.zeros((2 * rows, cols), dtype=CHAIN_IN_DTYPE)
    xx, ff, pp = np.zeros(rows * cols), np.zeros(rows * cols), np.zeros(rows * cols, dtype=np.int32)
    xx[:n], ff[:n], pp[:n] = x, f, p
    xx, ff, pp = xx.reshape(rows, cols), ff.reshape(rows, cols), pp.reshape(rows, cols).copy()
    pp[pp <= 0] = 1
    for r in range(1, rows):                                   # never the satellite of the pair above
        same = pp[r] == pp[r - 1]
        pp[r, same] = 1 + pp[r, same] % 32
    for k in (0, 1):
        cin["f_carr"][k::2], cin["carr_phase"][k::2], cin["prn"][k::2] = ff, xx, pp
    cin["carr_phase"][1::2] = 0.5                              # (never read: the second block continues the first)
    start, _, _ = gpsiq.reference_chain(cin, fs, nsamp)
    assert start[0::2].tobytes() == xx.tobytes()               # every pair did start from its own state
    return start[1::2].reshape(-1)[:n].copy()


# ---- link_block, restated on integers ---------------------------------------------------------------------------------------------
def _units_of(v):
    n, d = float(v).as_integer_ratio()
    return n * (_ONE // d)


def _float_of(y):
    if y == 0:
        return 0.0
    tz = (y & -y).bit_length() - 1
    return float(np.ldexp(float(y >> tz), tz - _K))


def _fits(y):
    """a double: at most 53 significant bits"""
    return y == 0 or y.bit_length() - ((y & -y).bit_length() - 1) <= 53


_units = np.frompyfunc(_units_of, 1, 1)
_floats = np.frompyfunc(_float_of, 1, 1)
_fit = np.frompyfunc(_fits, 1, 1)
WHY = ("admitted", "no map", "not a whole number of units", "outside lo..hi", "off the grid", "parity closed", "end not a double in [0, 1)")


def _link_big(rec, x):
    """link() on whole numbers of 2^-1074, which every double is: Python integers"""
    why = np.zeros(x.size, dtype=np.int8)
    diff = [int(a) - int(b) for a, b in zip(_units(x), _units(rec["xs"]))]
    whole = np.array([(v & ((1 << _SH) - 1)) == 0 for v in diff], dtype=bool)
    d = np.array([v >> _SH if w else 0 for v, w in zip(diff, whole)], dtype=np.int64)
    grid = (rec["info"] & 0xff).astype(np.int64)
    okgrid = (grid >= 1) & (grid <= 2)
    g = np.where(okgrid, grid, 1)
    p = (d >> (g - 1)) & 1
    k = d + np.where(p == 1, rec["cum"][:, 1], rec["cum"][:, 0])
    y_units = [int(e) + (int(v) << _SH) for e, v in zip(_units(rec["e"]), k)]
    fine = np.array([abs(int(kk)) <= (1 << 53) and 0 <= yy < _ONE and _fits(yy) for kk, yy in zip(k, y_units)], dtype=bool)
    for code, bad in ((6, ~fine), (5, ((rec["ok"] >> p) & 1) == 0), (4, ~okgrid | ((d & (g - 1)) != 0)), (3, (d < rec["lo"]) | (d > rec["hi"])),
                      (2, ~whole), (1, rec["ok"] == 0)):                  # the order link_block refuses in
        why[bad] = code
    y = np.array([_float_of(yy) if w == 0 else 0.0 for yy, w in zip(y_units, why)], dtype=np.float64)
    return why, d, y


_Q = 62                     # the quick way: states that are whole numbers of 2^-62 (all of them from 2^-10 up), on int64


def _quick(v):
    """v 2^62 where that is a whole number below 2^62 (a scaling by a power of two is exact, so is the test, so is the conversion)"""
    t = np.ldexp(v, _Q)
    good = (t == np.floor(t)) & (t >= 0.0) & (t < 2.0 ** _Q)
    return good, np.where(good, t, 0.0).astype(np.int64)


def _link_quick(rec, x, X, XS, E):
    why = np.zeros(x.size, dtype=np.int8)
    diff = X - XS
    sh = _Q - 53
    whole = (diff & ((1 << sh) - 1)) == 0
    d = np.where(whole, diff >> sh, 0)
    grid = (rec["info"] & 0xff).astype(np.int64)
    okgrid = (grid >= 1) & (grid <= 2)
    g = np.where(okgrid, grid, 1)
    p = (d >> (g - 1)) & 1
    k = d + np.where(p == 1, rec["cum"][:, 1], rec["cum"][:, 0])
    small = np.abs(k) <= (1 << 53)
    Y = E + (np.where(small, k, 0) << sh)                                 # below 2^63: no overflow
    fine = small & (Y >= 0) & (Y < (1 << _Q)) & (Y.astype(np.float64).astype(np.int64) == Y)     # a double: the conversion changes nothing
    for code, bad in ((6, ~fine), (5, ((rec["ok"] >> p) & 1) == 0), (4, ~okgrid | ((d & (g - 1)) != 0)), (3, (d < rec["lo"]) | (d > rec["hi"])),
                      (2, ~whole), (1, rec["ok"] == 0)):
        why[bad] = code
    y = np.where(why == 0, np.ldexp(Y.astype(np.float64), -_Q), 0.0)
    return why, d, y


def link(rec, x, quick=True):
    """lane::link_block for records rec (any shape) and start states x (broadcast against it) -> (why, d, y): why 0 where the
    map applies (WHY names the others), d the offset in units of U where it is a whole number (else 0), y the state after the block.
    On integers: exact_units(x, xs) says that x - xs is a whole number of U (then it is a double, the subtraction is exact, and it
    is far below 2^62 U); exact_shift(e, k) that |k| <= 2^53 and e + k U is a double; and link_block wants it in [0, 1)."""
    rec, x = np.broadcast_arrays(rec, np.asarray(x, dtype=np.float64))
    shape = x.shape
    rec, x = rec.reshape(-1), x.reshape(-1)
    why, d, y = np.zeros(x.size, dtype=np.int8), np.zeros(x.size, dtype=np.int64), np.zeros(x.size)
    (qx, X), (qs, XS), (qe, E) = _quick(x), _quick(rec["xs"]), _quick(rec["e"])
    q = qx & qs & qe & bool(quick)
    if q.any():
        why[q], d[q], y[q] = _link_quick(rec[q], x[q], X[q], XS[q], E[q])
    if not q.all():
        why[~q], d[~q], y[~q] = _link_big(rec[~q], x[~q])
    return why.reshape(shape), d.reshape(shape), y.reshape(shape)


def admits(rec, x):
    return link(rec, x)[0] == 0


def apply(rec, x):
    """the state after the block through the map (only where admits())"""
    return link(rec, x)[2]


# ---- the probes of a map ------------------------------------------------------------------------------------------------------------
FIXED = ("lo", "lo+grid", "hi", "hi-grid", "0", "lo/even", "hi/even", "0/even", "lo/odd", "hi/odd", "0/odd")


class Probes:
    """of maps rec[n]: d[n][P] offsets, x[n][P] = xs + d U, keep[n][P]; and what became of the others.  Columns: FIXED, then k
    uniform ones."""
    pass


def probes(rec, rng, k):
    """Start states to try for the maps rec[n] (ok != 0): offsets lo, lo + grid, hi, hi - grid and 0; for each parity ok allows
    the admissible offset nearest to lo, nearest to hi and nearest to 0; k uniform offsets in [lo, hi] on the grid.  A probe is
    KEPT if 0 <= x < 1 and admits(rec, x).  Of the others: `closed` are offsets the map itself does not claim (lo + grid of a map
    that holds for one parity only: the other parity's probes stand in), `skipped` the ones outside [0, 1) or refused by the
    exactness checks, which a true state cannot be either -- the ones the caps are about."""
    rec = np.atleast_1d(rec)
    n = rec.size
    lo, hi, ok = rec["lo"].astype(np.int64), rec["hi"].astype(np.int64), rec["ok"]
    grid = (rec["info"] & 0xff).astype(np.int64)
    assert np.all(ok != 0) and np.all((grid == 1) | (grid == 2))
    cols = [lo, lo + grid, hi, hi - grid, np.zeros(n, dtype=np.int64)]
    asked = [np.ones(n, dtype=bool)] * 5
    for p in (0, 1):
        has = ((ok >> p) & 1) == 1
        first = lo + np.mod(p * grid - lo, 2 * grid)                 # the first offset >= lo that is p (mod 2) grid steps
        last = hi - np.mod(hi - p * grid, 2 * grid)
        zero = np.zeros(n, dtype=np.int64) if p == 0 else np.where(grid <= hi, grid, -grid)
        cols += [first, last, zero]
        asked += [has & (first <= hi), has & (last >= lo), has & (zero >= lo) & (zero <= hi)]
    lo_g, hi_g = lo + np.mod(-lo, grid), hi - np.mod(hi, grid)
    steps = np.maximum((hi_g - lo_g) // grid, 0)
    for _ in range(k):
        u = lo_g + grid * np.floor(rng.random(n) * (steps + 1)).astype(np.int64)
        # onto a parity the map holds for
        par = (u // grid) & 1
        u = np.where(((ok >> par) & 1) == 1, u, np.where(u + grid <= hi, u + grid, u - grid))
        cols.append(u)
        asked.append(lo_g <= hi_g)
    P = Probes()
    P.d = np.stack(cols, axis=1)
    ask = np.stack(asked, axis=1)
    order = list(range(5, 11)) + list(range(5)) + list(range(11, P.d.shape[1]))
    for n_, j in enumerate(order):                                    # an offset asked for twice is tried once (under its parity's name)
        for i in order[:n_]:
            ask[:, j] &= ~((P.d[:, i] == P.d[:, j]) & ask[:, i])
    P.x = rec["xs"][:, None] + P.d.astype(np.float64) * U
    inside = (P.x >= 0.0) & (P.x < 1.0)
    P.why = np.full(P.d.shape, -1, dtype=np.int8)
    sel = ask & inside
    why, dd, yy = link(np.broadcast_to(rec[:, None], P.d.shape)[sel], P.x[sel])
    why = np.where((why == 0) & (dd != P.d[sel]), 2, why)            # (xs + d U was rounded: not the state that was meant)
    P.why[sel] = why
    P.y = np.zeros(P.d.shape)
    P.y[sel] = yy
    P.moved = 0
    # "the admissible offset nearest to lo / hi": where the exactness checks refuse the end itself (beyond it xs + d U or the end
    # state leaves the binade whose grid it lies on), the refused end counts as skipped and the nearest offset that IS admitted,
    # found by bisection from the parity's probe at 0, is tried in its place
    for col in (5, 6, 8, 9):
        zero = 7 if col < 8 else 10
        for m in np.flatnonzero(sel[:, col] & np.isin(P.why[:, col], (2, 6))):
            a, b, step = int(P.d[m, zero]), int(P.d[m, col]), 2 * int(grid[m])
            if not (lo[m] <= a <= hi[m]) or link(rec[m], rec["xs"][m] + a * U)[0] != 0:
                continue
            while abs(b - a) > step:
                mid = a + ((b - a) // (2 * step)) * step
                if mid == a:
                    mid = a + (step if b > a else -step)
                w, dm, _ = link(rec[m], rec["xs"][m] + mid * U)
                if w == 0 and dm == mid:
                    a = mid
                else:
                    b = mid
            j = P.d.shape[1] - 1 - P.moved % max(k, 1) if k else None
            if j is None:
                continue
            # (takes the place of one of this map's uniform probes)
            P.d[m, j], P.x[m, j] = a, rec["xs"][m] + a * U
            w, _, y1 = link(rec[m], P.x[m, j])
            P.why[m, j], P.y[m, j], ask[m, j], sel[m, j], inside[m, j] = w, y1, True, True, True
            P.d[m, col] = b if P.why[m, col] != 0 else P.d[m, col]
            P.ends = getattr(P, "ends", []) + [(m, col, j)]
    P.keep = P.why == 0
    P.closed = sel & np.isin(P.why, (3, 4, 5))
    P.skipped = (ask & ~inside) | (sel & np.isin(P.why, (2, 6)))
    P.asked, P.inside = ask, inside
    return P


# ---- the audit ------------------------------------------------------------------------------------------------------------------------
class Audit:
    """counts and the population of one audit() (add them up with +)"""
    FIELDS = ("maps", "kept", "skipped", "closed", "ok1", "ok2", "ok3", "cum_differ", "grid1", "grid2", "c_pos", "c_neg",
              "odd_at_lo", "odd_at_hi", "ends_short")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, int(kw.get(f, 0)))
        self.seg = set(kw.get("seg", ()))

    def __add__(self, o):
        r = Audit(**{f: getattr(self, f) + getattr(o, f) for f in self.FIELDS})
        r.seg = self.seg | o.seg
        return r

    def __repr__(self):
        return "Audit(" + ", ".join(f"{f}={getattr(self, f)}" for f in self.FIELDS) + f", stretches={sorted(self.seg)})"

    def assert_caps(self):
        """B.4, the two caps: skipped probes at most 10 % of those generated; every map keeps its lo-side and hi-side probe of
        one parity unless that end lies outside [0, 1)"""
        assert self.skipped <= 0.10 * (self.kept + self.skipped), self
        assert self.ends_short == 0, self


def audit(cin, maps, fs, nsamp, rng, k, max_stretches=None):
    """For every block with ok != 0 and every kept probe: apply(rec, x) == the serial end, bit for bit -- walk() where
    nsamp <= 4096, serial_end() otherwise.  -> Audit"""
    cin, maps = np.asarray(cin), np.asarray(maps)
    at = np.argwhere(maps["ok"] != 0)
    if not len(at):
        return Audit()
    blk, slot = at[:, 0], at[:, 1]
    rec, d = maps[blk, slot], cin[blk, slot]
    assert np.all(d["prn"] > 0), "a map for an unused block"
    c = d["f_carr"] * (1.0 / fs)
    P = probes(rec, rng, k)
    m, j = np.nonzero(P.keep)
    x = P.x[m, j]
    got = P.y[m, j]
    want = walk(x, c[m], nsamp) if nsamp <= WALK_MAX else serial_end(x, d["prn"][m], d["f_carr"][m], fs, nsamp)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    if len(bad):
        q = bad[0]
        r = rec[m[q]]
        raise AssertionError(
            f"{len(bad)} of {len(x)} probes end elsewhere than their map says; the first: block {blk[m[q]]} slot {slot[m[q]]} c {c[m[q]].hex()} "
            f"xs {float(r['xs']).hex()} d {P.d[m[q], j[q]]} ({(FIXED + ('uniform',) * k)[j[q]]}) lo {r['lo']} hi {r['hi']} ok {r['ok']} info {r['info']:#x} "
            f"cum {r['cum'].tolist()} got {got[q].hex()} want {want[q].hex()}")
    # a map's ends: its lo-side and hi-side probe of one parity kept, unless that end lies outside [0, 1)
    short = np.zeros(len(rec), dtype=bool)
    odd_lo = odd_hi = 0
    for side, cols in (("lo", (5, 8)), ("hi", (6, 9))):
        fine = np.zeros(len(rec), dtype=bool)
        for col in cols:
            dup = ~P.asked[:, col] & np.any((P.d == P.d[:, col:col + 1]) & P.keep, axis=1)       # (tried under another name)
            has = ((rec["ok"] >> (0 if col < 8 else 1)) & 1) == 1
            fine |= has & (P.keep[:, col] | dup | ~P.inside[:, col])
            for mm, cc, jj in getattr(P, "ends", []):                  # the end was refused as no double: the nearest admitted offset stands in
                if cc == col and P.keep[mm, jj]:
                    fine[mm] = True
        short |= ~fine
        kept_odd = (P.keep[:, cols[1]] | (~P.asked[:, cols[1]] & np.any((P.d == P.d[:, cols[1]:cols[1] + 1]) & P.keep, axis=1))) & (((rec["ok"] >> 1) & 1) == 1)
        if side == "lo":
            odd_lo = int(kept_odd.sum())
        else:
            odd_hi = int(kept_odd.sum())
    seg = set(np.unique(stretches(c, nsamp, max_stretches)).tolist()) if max_stretches else ()
    return Audit(maps=len(rec), kept=len(x), skipped=P.skipped.sum(), closed=P.closed.sum(), ok1=(rec["ok"] == 1).sum(), ok2=(rec["ok"] == 2).sum(),
                 ok3=(rec["ok"] == 3).sum(), cum_differ=(rec["cum"][:, 0] != rec["cum"][:, 1]).sum(), grid1=((rec["info"] & 0xff) == 1).sum(),
                 grid2=((rec["info"] & 0xff) == 2).sum(), c_pos=(c > 0).sum(), c_neg=(c < 0).sum(), odd_at_lo=odd_lo, odd_at_hi=odd_hi,
                 ends_short=short.sum(), seg=seg)


# ---- what the chain tests check besides ------------------------------------------------------------------------------------------------
def true_admission(maps, cin, true_start):
    """admits(rec, true start) for every block -> bool [nblocks][nchan] (False where the slot is unused)"""
    act = cin["prn"] > 0
    out = np.zeros(cin.shape, dtype=bool)
    out[act] = admits(maps[act], true_start[act])
    return out


def event_blocks(record, shape):
    """the engineered-event blocks and the blocks after them -> bool [nblocks][nchan]"""
    m = np.zeros(shape, dtype=bool)
    for e in record:
        for b in (e["block"], e["block"] + 1):
            if 0 <= b < shape[0]:
                m[b, e["slot"]] = True
    return m


def expected_device_flags(end_host, start, cin):
    """gpsiq_plumbing.h on gpsiq_chain_maps_device: EXACT never set; RESEEDED as the host sets it, and also where block 0
    continued an exact state handed in through `start`"""
    f = end_host["flags"] & CHAIN_RESEEDED
    if start is not None and cin.shape[0]:
        cont = ((start["flags"] & CHAIN_EXACT) != 0) & (start["prn"] == cin["prn"][0]) & (cin["prn"][0] > 0)
        f = np.where(cont, f | CHAIN_RESEEDED, f)
    return f


# ---- timelines ------------------------------------------------------------------------------------------------------------------------
FS = 2.6e6
FS_TIE = 2097152.0          # 2^21: c = f_carr / 2^21 keeps f_carr's mantissa, trailing zeros included
NC = 16                     # every timeline is built 16 slots wide; a case with fewer channels runs it in column groups (slots are independent)


def _base(nb, nsamp, fs, seed, cyc=(0.55, 0.95)):
    """ordinary slots: Doppler ramps with |c| nsamp in cyc[0..1] x C_MAX nsamp, signs alternating, a fresh carr_phase in every block"""
    rng = np.random.default_rng(seed)
    cin = np.zeros((nb, NC), dtype=CHAIN_IN_DTYPE)
    b = np.arange(nb)
    for i in range(NC):
        f0 = rng.uniform(cyc[0], cyc[1]) * C_MAX * fs * (1 if i % 2 == 0 else -1)
        df = rng.uniform(-0.4, 0.4) * min(1.0, 200.0 / max(nb, 1))
        cin["f_carr"][:, i] = f0 + df * b + rng.uniform(-0.02, 0.02, nb)
        cin["prn"][:, i] = 1 + (3 * i + seed) % 32
    cin["carr_phase"] = rng.random((nb, NC))
    return cin, rng


def _other(prn):
    return 1 + prn % 32


def _zigzag(nb, at, slope, half, cap):
    """Doppler that changes sign at every position of `at`: exactly zero on block p (half = 0), or between p - 1 and p (half = 0.5)"""
    b = np.arange(nb, dtype=np.float64)
    at = sorted(at)
    if not at:
        return None
    edges = [-np.inf] + [(p + q) / 2.0 for p, q in zip(at[:-1], at[1:])] + [np.inf]
    f = np.zeros(nb)
    for k, p in enumerate(at):
        seg = (b >= edges[k]) & (b < edges[k + 1])
        f[seg] = (1 if k % 2 == 0 else -1) * np.clip(slope * (b[seg] - p + half), -cap, cap)
    return f


SCAN_POSITIONS = (K_WAVE - 1, K_WAVE, K_PREP_THREADS - 1, K_PREP_THREADS, 2 * K_PREP_THREADS - 1, 2 * K_PREP_THREADS)
SCAN_BLOCKS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)


def scan_edge_timeline(nb, nsamp=600, fs=FS, seed=1):
    """chain_prepare's scan edges: the last thread of a wave and the first of the next (63 / 64), the last block of a round and the
    first of the next (1023 / 1024, 2047 / 2048).  Slots 0-7: a satellite change, an unused run beginning, an unused run ending
    and Doppler through zero ON those blocks (two slots per kind: the positions 63, 1023, 2047 in one, 64, 1024, 2048 in the other);
    slot 8 unused for a whole wave (64..127) and a whole round (1024..2047); slot 9 unused on the last block of a round and on the
    final block; slot 10 never used; slots 11-15 ordinary.  -> (cin, record)"""
    cin, rng = _base(nb, nsamp, fs, seed + nb)
    rec = []
    for par in (0, 1):
        pos = [p for p in SCAN_POSITIONS[par::2] if 1 <= p < nb]
        for p in pos:
            s = 0 + par
            cin["prn"][p:, s] = _other(int(cin["prn"][p - 1, s]))
            rec.append(dict(kind="change", slot=s, block=p))
            s = 2 + par
            cin["prn"][p:p + 3, s] = 0
            rec.append(dict(kind="unused_begins", slot=s, block=p))
            s = 4 + par
            cin["prn"][max(p - 2, 0):p + 1, s] = 0
            rec.append(dict(kind="unused_ends", slot=s, block=p))
            rec.append(dict(kind="doppler_zero" if par == 0 else "doppler_sign", slot=6 + par, block=p))
        f = _zigzag(nb, pos, 0.002 * C_MAX * fs, 0.0 if par == 0 else 0.5, 0.9 * C_MAX * fs)
        if f is not None:
            cin["f_carr"][:, 6 + par] = f
    for lo, hi, kind in ((K_WAVE, 2 * K_WAVE, "unused_wave"), (K_PREP_THREADS, 2 * K_PREP_THREADS, "unused_round")):
        if hi < nb:
            cin["prn"][lo:hi, 8] = 0
            rec.append(dict(kind=kind, slot=8, block=lo))
            rec.append(dict(kind=kind + "_back", slot=8, block=hi))
    if K_PREP_THREADS < nb:
        cin["prn"][K_PREP_THREADS - 3:K_PREP_THREADS, 9] = 0
        rec.append(dict(kind="unused_round_end", slot=9, block=K_PREP_THREADS - 1))
    cin["prn"][nb - 1, 9] = 0
    rec.append(dict(kind="unused_final", slot=9, block=nb - 1))
    cin["prn"][:, 10] = 0
    rec.append(dict(kind="never_used", slot=10, block=0))
    return cin, rec


NS_LANES = 9600             # |c| < 2^-6: a block of 32 stretches (128 cycles) has more than 8192 samples
LANE_SEGS = {4: (1, 2, 4), 8: (5, 8), 16: (9, 16), 32: (17, 31, 32)}          # kSeg -> the max_stretches that reach it


def lane_positions(kseg, nb):
    kb = K_LANE_THREADS // kseg
    return [w for g in (1, 2, 3) for w in (g * kb - 1, g * kb) if 1 <= w < nb]


def lane_blocks(kseg):
    kb = K_LANE_THREADS // kseg
    return (kb - 1, kb, kb + 1, 3 * kb + 1)


def lane_edge_timeline(kseg, nb, nsamp=NS_LANES, fs=FS, seed=2):
    """chain_lanes<kseg>'s workgroup edges (every 256 / kseg blocks): on the first block of a workgroup and on the last one before
    it (two slots per kind), a satellite change (0, 1), an unused block before it (2, 3), a Doppler sign change (4, 5), and an
    addend the walk does not take in the block BEFORE it (6, 7: c == 0, |c| < 2^-22, |c| >= 2^-6 in turn).  Slot 8: blocks of one
    stretch (|c| nsamp < 8) next to blocks of 32; slots 9-11: |c| nsamp about 60, about 70, and the two in turn (the table
    threshold 64); slots 12-15 ordinary.  -> (cin, record)"""
    cin, rng = _base(nb, nsamp, fs, seed + 7 * kseg + nb, cyc=(0.86, 0.98))
    kb = K_LANE_THREADS // kseg
    rec = []
    bad = (0.0, 0.5 * C_MIN * fs, 1.3 * C_MAX * fs)
    for par in (0, 1):                                              # 0: the last block before a workgroup, 1: the first of one
        pos = [w for w in lane_positions(kseg, nb) if (w % kb == 0) == (par == 1)]
        for n, w in enumerate(pos):
            cin["prn"][w:, 0 + par] = _other(int(cin["prn"][w - 1, 0 + par]))
            rec.append(dict(kind="change", slot=0 + par, block=w))
            cin["prn"][w - 1, 2 + par] = 0
            rec.append(dict(kind="unused_before", slot=2 + par, block=w))
            rec.append(dict(kind="doppler_sign", slot=4 + par, block=w))
            cin["f_carr"][w - 1, 6 + par] = bad[n % 3] * (1 if n % 2 else -1)
            rec.append(dict(kind="addend_not_walked_before", slot=6 + par, block=w, which=n % 3))
        f = _zigzag(nb, pos, 0.05 * C_MAX * fs, 0.5, 0.95 * C_MAX * fs)
        if f is not None:
            cin["f_carr"][:, 4 + par] = f + rng.uniform(-0.02, 0.02, nb)
    if 75.0 / nsamp >= C_MAX:                                       # (nsamp 1 and 7: no addend the lanes walk makes that many cycles)
        return cin, rec
    b = np.arange(nb)
    one = 6.0 / nsamp * fs                                           # 6 cycles a block: one stretch
    cin["f_carr"][:, 8] = np.where(b % 3 == 1, one, cin["f_carr"][:, 8])
    for s, cyc in ((9, np.full(nb, 60.0)), (10, np.full(nb, 70.0)), (11, np.where(b % 2 == 0, 60.0, 70.0))):
        cin["f_carr"][:, s] = (cyc + rng.uniform(-1.0, 1.0, nb)) / nsamp * fs * (1 if s != 10 else -1)
    for s in (8, 9, 10, 11):
        rec.append(dict(kind="stretch_mix" if s == 8 else "table_threshold", slot=s, block=0, nsamp=nsamp))
    return cin, rec


TIE_BITS = (-53, -54, -55, -52)


def tie_timeline(nb, nsamp, seed=3, fs=FS_TIE):
    """Exact ties: at fs = 2^21 the addend has f_carr's mantissa, so its trailing zeros are f_carr's (mode 4 of
    tests/chain_parallel.cpp).  An addend whose LOWEST bit is 2^-53 is, added to a post-wrap state, half way between two states of
    [1, 2) on every other wrap (a positive addend's sigma); 2^-54 is the tie of [0.5, 1): a descending carrier's top tie (even
    offsets only), a climbing one's tie binade; 2^-55 the binade below; 2^-52: no tie, for comparison.  Slot i: sign by i % 2, lowest
    bit TIE_BITS[(i // 2) % 4]; slot 11 (descending, 2^-54) makes six cycles a block.  -> (cin, record)"""
    cin, rng = _base(nb, nsamp, fs, seed + nb, cyc=(0.80, 0.98))
    rec = []
    cin["f_carr"][:, 11] = -(6.0 + rng.random(nb)) / nsamp * fs          # one stretch whatever max_stretches is: a top tie's map holds (for even offsets)
    bits = cin["f_carr"].view(np.uint64).copy()
    one = np.uint64(1)
    for i in range(NC):
        t = TIE_BITS[(i // 2) % 4]
        ec = ((bits[:, i] >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 21       # c = f_carr / 2^21
        z = (t + 1075 - ec).astype(np.uint64)                                                # ulp(c) = 2^(ec - 1075)
        bits[:, i] = (bits[:, i] & ~((one << z) - one)) | (one << z)
        rec.append(dict(kind="tie", slot=i, block=0, bit=t))
    cin["f_carr"] = bits.view(np.float64)
    return cin, rec


def parts(cin, record, nchan):
    """a 16-slot timeline in column groups of nchan slots: [(cin[:, group], record of the group with its slots renumbered)]"""
    out = []
    for s0 in range(0, cin.shape[1], nchan):
        s1 = min(s0 + nchan, cin.shape[1])
        out.append((np.ascontiguousarray(cin[:, s0:s1]), [dict(e, slot=e["slot"] - s0) for e in record if s0 <= e["slot"] < s1]))
    return out


def check_record(cin, record, fs):
    """every engineered event sits on the block it was meant for (what the kinds mean, read off the timeline itself)"""
    prn, c = cin["prn"], cin["f_carr"] * (1.0 / fs)
    nb = cin.shape[0]
    for e in record:
        s, b, kind = e["slot"], e["block"], e["kind"]
        if kind == "change":
            assert prn[b, s] > 0 and prn[b - 1, s] > 0 and prn[b, s] != prn[b - 1, s], e
        elif kind in ("unused_begins", "unused_wave", "unused_round"):
            assert prn[b, s] == 0 and prn[b - 1, s] > 0, e
            if kind != "unused_begins":
                n = K_WAVE if kind == "unused_wave" else K_PREP_THREADS
                assert np.all(prn[b:b + n, s] == 0) and b % n == 0, e
        elif kind == "unused_ends":
            assert prn[b, s] == 0 and (b + 1 >= nb or prn[b + 1, s] > 0), e
        elif kind == "unused_round_end":
            assert prn[b, s] == 0 and (b + 1) % K_PREP_THREADS == 0 and b + 1 < nb, e
        elif kind in ("unused_wave_back", "unused_round_back"):
            assert prn[b, s] > 0 and prn[b - 1, s] == 0, e
        elif kind == "unused_final":
            assert b == nb - 1 and prn[b, s] == 0, e
        elif kind == "never_used":
            assert np.all(prn[:, s] == 0), e
        elif kind == "unused_before":
            assert prn[b, s] > 0 and prn[b - 1, s] == 0 and (b < 2 or prn[b - 2, s] > 0), e
        elif kind == "doppler_zero":
            assert c[b, s] == 0.0 and c[b - 1, s] * (c[b + 1, s] if b + 1 < nb else -c[b - 1, s]) < 0.0, e
        elif kind == "doppler_sign":
            assert c[b, s] * c[b - 1, s] < 0.0 and walked_by_lanes(c[b, s]) and walked_by_lanes(c[b - 1, s]), e
        elif kind == "addend_not_walked_before":
            assert not walked_by_lanes(c[b - 1, s]) and walked_by_lanes(c[b, s]) and prn[b, s] == prn[b - 1, s] > 0, e
            assert (c[b - 1, s] == 0.0, 0 < abs(c[b - 1, s]) < C_MIN, abs(c[b - 1, s]) >= C_MAX)[e["which"]], e
        elif kind == "stretch_mix":
            cyc = np.abs(c[:, s]) * e.get("nsamp", NS_LANES)
            assert nb < 2 or ((cyc < 8).any() and (cyc >= 128).any()), e
        elif kind == "table_threshold":
            cyc = np.abs(c[:, s]) * e.get("nsamp", NS_LANES)
            assert np.all((cyc > 55) & (cyc < 75)) and np.all(np.abs(cyc - 2 * K_ENTRIES_HOST) > 2), e
        elif kind == "tie":
            m, ex = np.frexp(c[:, s])
            M = np.ldexp(np.abs(m), 53).astype(np.int64)
            low = ex - 53 + np.log2((M & -M).astype(np.float64)).astype(np.int64)          # the exponent of c's lowest bit
            assert np.all(low == e["bit"]) and np.all(walked_by_lanes(c[:, s])), e
        else:
            raise AssertionError(f"unknown kind {kind}")
