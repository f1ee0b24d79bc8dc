"""The cases that hold the stream stages to the clauses of include/gpsiq_rows.h and include/gpsiq.h that are not arithmetic: stream
order (tests/test_gpu_stage_streams.py), offsets past 2^31 and 2^32 (tests/test_gpu_wide_offsets.py), the lowest shift on a tie
(tests/test_gpu_acquire.py) and 32 followed satellites on a used context (tests/test_gpu_follow_lifecycle.py).  Every reference is
computed once per process and never written to.  tests/test_stage_contract_cases.py holds the cases to their names on the CPU.
TEST INFRASTRUCTURE."""
import collections
import functools

import numpy as np

import _acquire_plan as ap
import _acquire_ref as ar
import _despread_plan as dp
import _despread_ref as dr
import _follow_plan as fp
import _follow_ref as fr
import _oracle
import _pack_ref as pr
from gpsiq.abi import FOLLOW_STATE_DTYPE, SC08, SC16, elem_dtype

GUARD = 0x7F


def by_name(table, name):
    return [c for c in table if c.name == name][0]


def guard_elements(count, ss):
    """`count` elements of a buffer filled with 0x7f: 127 in int8, 0x7f7f in int16"""
    return np.full(count, GUARD, dtype=np.uint8).repeat(ss).view(elem_dtype(ss))


# ---- A. stream order ----------------------------------------------------------------------------------------------------------------
# Cases of the existing tables, with the streams their own GPU tests give them.  *_reference: what the stage must return for the true
# input; *_of_guard: what it returns for the 0x7f bytes the buffer holds until the producer on the side stream has run.
STREAM_DESPREAD = ("both-rows", "both-generic")
STREAM_ACQUIRE = ("rows-d6-ss1", "k3-h129-generic-shape")
STREAM_FOLLOW = ("mixed-int16",)
STREAM_FOLLOW_KNOB = 7
STREAM_PACK_BLOCKS, STREAM_PACK_NSAMP = 5, 70001
PACK_FORMATS = [(ss, bits) for ss in (SC08, SC16) for bits in (pr.PK4, pr.PK2)]
DESPREAD_CLIP = {SC08: 100, SC16: 30000}


@functools.lru_cache(maxsize=None)
def despread_reference(name):
    """(case, descriptors, stream [nblocks][2 nsamp], (sums, prn, stats)): the stream of tests/test_gpu_despread.py's test_case_table"""
    from test_gpu_despread import case_descriptors, random_stream
    c = by_name(dp.CASES, name)
    q = case_descriptors(c)
    stream = random_stream(np.random.default_rng(dp.CASES.index(c)), c.nblocks, c.nsamp, c.ss)
    stream.setflags(write=False)
    return c, q, stream, _despread(c, q, stream)


def _despread(c, q, stream):
    sums, prn = dr.despread(_oracle.load_oracle(), q[c.block0:c.block0 + c.nblocks], stream, c.nsamp, c.seg_len)
    return sums, prn, dr.stats(stream, c.nsamp, DESPREAD_CLIP[c.ss])


@functools.lru_cache(maxsize=None)
def despread_of_guard(name):
    c, q, _, _ = despread_reference(name)
    return _despread(c, q, guard_elements(c.nblocks * 2 * c.nsamp, c.ss).reshape(c.nblocks, -1))


def acquire_reference(name):
    """(stream, steps, (peaks, power, corr)) as tests/test_gpu_acquire.py caches it"""
    from test_gpu_acquire import case_reference
    return case_reference(name)


@functools.lru_cache(maxsize=None)
def acquire_of_guard(name):
    c = by_name(ap.CASES, name)
    stream, steps, _ = acquire_reference(name)
    return ar.acquire(_oracle.load_oracle(), guard_elements(len(stream), c.ss), c.prns, *steps, c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop)


def follow_reference(name):
    """(case, stream, cfg, states, (records, nepochs, states out)) as tests/test_gpu_follow.py caches it"""
    from test_gpu_follow import case_reference
    return case_reference(name)


@functools.lru_cache(maxsize=None)
def follow_of_guard(name):
    c, stream, cfg, states, _ = follow_reference(name)
    return fr.follow(_oracle.load_oracle(), guard_elements(len(stream), c.ss), cfg, states, c.max_epochs)


@functools.lru_cache(maxsize=None)
def pack_reference(ss, bits):
    """(elements [5][2 * 70001] of random bytes, packed bytes, clamp count, the packed bytes unpacked again)"""
    nb, n = STREAM_PACK_BLOCKS, STREAM_PACK_NSAMP
    x = np.random.default_rng(5100 + 10 * ss + bits).integers(0, 256, size=(nb, 2 * n * ss), dtype=np.uint8).view(elem_dtype(ss))
    packed, count = pr.pack(x, bits)
    back = pr.unpack(packed, n, bits, elem_dtype(ss))
    for a in (x, packed, back):
        a.setflags(write=False)
    return x, packed, count, back


def pack_of_guard(ss, bits):
    """(packed bytes, clamp count) of a source of 0x7f bytes, and the elements a packed stream of 0x7f bytes unpacks to"""
    nb, n = STREAM_PACK_BLOCKS, STREAM_PACK_NSAMP
    packed, count = pr.pack(guard_elements(nb * 2 * n, ss).reshape(nb, -1), bits)
    return packed, count, pr.unpack(np.full((nb, pr.packed_block_bytes(n, bits)), GUARD, dtype=np.uint8), n, bits, elem_dtype(ss))


# ---- B. offsets past 2^31 and 2^32 --------------------------------------------------------------------------------------------------
WIDE_STRIDE = 2 ** 30 + 4          # bytes between blocks: block 2 starts at 2^31 + 8, block 4 at 2^32 + 16
WIDE_BLOCKS = 5
WIDE_TAIL = 64


def wide_bytes(block_bytes):
    """bytes of a buffer that holds five blocks WIDE_STRIDE apart and a tail behind the last"""
    return (WIDE_BLOCKS - 1) * WIDE_STRIDE + block_bytes + WIDE_TAIL


WideSearch = collections.namedtuple("WideSearch", "name ss nsamp prns ndopp nshift ncoh nnoncoh hop seed")


def _wide_search(name, ss, nsamp, seed):
    nshift, ncoh = 300, 128
    return WideSearch(name, ss, nsamp, (9, 27), 3, nshift, ncoh, 2, nsamp - (nshift - 1) - ncoh, seed)


# the second dwell ends on the span's last sample: 4.8e9 bytes in for int16, element indices past 2^31 for int8
WIDE_SEARCHES = (_wide_search("int16", SC16, 1200000000, 8101), _wide_search("int8", SC08, 2 ** 31 - 1, 8102))
WIDE_STEPS = ar.steps(2.6e6, -500.0, 500.0)


def wide_windows(w):
    """the two dwell windows of a wide search (random elements, the format's extremes at either end of each) and their first samples"""
    info = np.iinfo(elem_dtype(w.ss))
    rng = np.random.default_rng(w.seed)
    width = w.nshift - 1 + w.ncoh
    wins = []
    for _ in range(w.nnoncoh):
        x = rng.integers(info.min, info.max + 1, size=2 * width).astype(elem_dtype(w.ss))
        x[:2], x[-2:] = info.min, info.max
        wins.append(x)
    return wins, [k * w.hop for k in range(w.nnoncoh)]


@functools.lru_cache(maxsize=None)
def wide_search_reference(name):
    w = by_name(WIDE_SEARCHES, name)
    wins, first = wide_windows(w)
    return w, wins, first, ar.acquire_windows(_oracle.load_oracle(), wins, first, w.prns, *WIDE_STEPS, w.ndopp, w.nshift, w.ncoh)


# follow on the int16 span of the wide search: two satellites that start some 3000 samples before its end
WIDE_FOLLOW_MAX_EPOCHS = 8


@functools.lru_cache(maxsize=None)
def wide_follow_reference():
    """(nsamp, first sample of the tail, tail elements, cfg, states, (records, nepochs, states out)).  The span is the int16 search's up to
    its second dwell window (so both fit one buffer), the tail its last samples: random elements cut so that satellite 0's fourth
    record ends on the span's last sample; the rest of the span is never read."""
    orc = _oracle.load_oracle()
    nsamp = WIDE_SEARCHES[0].hop
    info = np.iinfo(np.int16)
    raw = np.random.default_rng(8103).integers(info.min, info.max + 1, size=2 * 4096).astype(np.int16)
    cfg = fr.make_cfg(**fp.LOOP)
    local = [fr.make_state(11, sample=100, code_step=fp.C15, carr_step=-(1 << 50)),
             fr.make_state(24, sample=7, chip=300, code_frac=98765, code_step=fp.C15, carr_step=123456789012345)]
    rec, n, _ = fr.follow(orc, raw, cfg, local[:1], 4)
    assert n[0] == 4
    end = int(rec[0, 3]["sample"]) + int(rec[0, 3]["nsamp"])
    tail = raw[:2 * end].copy()
    tail[-2:] = info.max
    tail.setflags(write=False)
    base = nsamp - end
    states = np.array(local, dtype=FOLLOW_STATE_DTYPE)
    states["sample"] += np.uint64(base)
    return nsamp, base, tail, cfg, states, fr.follow_rebased(orc, tail, base, cfg, states, WIDE_FOLLOW_MAX_EPOCHS)


# ---- C. peak ties -------------------------------------------------------------------------------------------------------------------
# carr_step0 = 0: bin 0 wipes every sample with table entry 0, so a stream of period P samples gives X(s + P) = X(s) exactly, for every
# dwell and any hop, and equal power bits.  Bin 1 (500 Hz) has no such symmetry.
Tie = collections.namedtuple("Tie", "name ss period nshift ncoh nnoncoh hop prns ndopp seed")
TIES = (Tie("p100-int16", SC16, 100, 700, 128, 2, 333, (4, 21), 2, 3),
        Tie("p64-int8", SC08, 64, 300, 64, 1, 64, (4, 21), 2, 2),          # ties in one lane across iterations
        Tie("p16-int16", SC16, 16, 257, 64, 3, 50, (4, 21), 2, 1))         # ties across lanes and tiles
TIE_STEPS = ar.steps(2.6e6, 0.0, 500.0)


def tie_stream(t):
    info = np.iinfo(elem_dtype(t.ss))
    one = np.random.default_rng(t.seed).integers(info.min, info.max + 1, size=2 * t.period).astype(elem_dtype(t.ss))
    nsamp = ap.span_of(t.nshift, t.ncoh, t.nnoncoh, t.hop)
    return np.tile(one, -(-nsamp // t.period))[:2 * nsamp].copy()


@functools.lru_cache(maxsize=None)
def tie_reference(name):
    """(case, stream, (peaks, power, corr))"""
    t = by_name(TIES, name)
    stream = tie_stream(t)
    stream.setflags(write=False)
    return t, stream, ar.acquire(_oracle.load_oracle(), stream, t.prns, *TIE_STEPS, t.ndopp, t.nshift, t.ncoh, t.nnoncoh, t.hop)


# ---- D. thirty-two satellites -------------------------------------------------------------------------------------------------------
FOLLOW32_KNOB = 5
FOLLOW32_CFG = dict(fp.LOOP, kd=(1 << 46) - 1)              # the gain of _follow_plan's range-code: a code step next to its limit leaves it
# statuses of the 32 satellites at 12 epochs, by format (tests/test_stage_contract_cases.py pins them against the restatement)
_E32 = (2,) + (1,) * 4 + (3,) + (1,) * 14 + (3,) + (1,) * 11
FOLLOW32_EXPECT = {SC08: _E32, SC16: _E32}


def follow32_states():
    """one state per PRN 1..32: starts 250 samples apart (so that the span ends them at different epochs), chips and fractions spread
    over their ranges, carrier steps of both signs; PRN 6 and 21 start with the code step next to its upper limit"""
    out = []
    for p in range(32):
        near = p in (5, 20)
        out.append(fr.make_state(p + 1, sample=250 * p + p % 3, chip=(37 * p) % 1023, code_frac=(p * 0x123456789ABCD) & fp.TOP56,
                                 code_step=(1 << 57) - 1000 if near else fp.C15, carr_step=(-1) ** p * ((p + 1) << 44)))
    return np.array(out, dtype=FOLLOW_STATE_DTYPE)


@functools.lru_cache(maxsize=None)
def follow32_reference(ss, nsamp=9000, max_epochs=12):
    """(stream, cfg, states, (records, nepochs, states out)); 9000 samples hold 12 epochs of 682 for the first satellites only"""
    info = np.iinfo(elem_dtype(ss))
    stream = np.random.default_rng(3200 + ss).integers(info.min, info.max + 1, size=2 * nsamp).astype(elem_dtype(ss))
    stream[:2], stream[-2:] = info.min, info.max
    stream.setflags(write=False)
    cfg, states = fr.make_cfg(**FOLLOW32_CFG), follow32_states()
    return stream, cfg, states, fr.follow(_oracle.load_oracle(), stream, cfg, states, max_epochs)
