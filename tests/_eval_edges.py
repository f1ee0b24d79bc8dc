"""Timelines and references for the edges of the device-evaluated batch call (csrc/gpsiq_evaldev.cpp, gpsiq_eval_kernels.hip):
descriptors whose events -- a slot that changes satellite, goes unused, comes back -- sit on and next to the block indices where
the scan kernels hand a carry on (chain_link_scan: every 256 blocks; carry_prefix: every 4 blocks of a thread, every 256 of a wave,
every 1 024 of a round; every piece of a call), and the two references the GPU tests compare every byte with.  Pure numpy and the
oracle (oracle/liboracle.so): nothing here calls libgpsiq, and nothing needs a GPU.  tests/test_eval_edges.py
holds this module to the descriptors it builds and to the library's serial chain; tests/test_gpu_eval_edges.py uses it.

A timeline comes with a RECORD of what was put where: {"placed": [event, ...], "deferred": [key, ...], "outside": [key, ...]}.
An event is a dict with "key" (kind, boundary[, offset]), "slot" and the blocks it touches; "deferred" are the events that found no
slot in this part of the timeline (they are placed in a later part: edge_timelines() returns every part), "outside" the ones
that do not exist for this boundary and length (a change at block 0 is not a change).  Nothing is dropped silently: every event
edge_events() lists is in exactly one of the three, and over all parts every one that exists is placed."""
import numpy as np

from gpsiq.abi import elem_dtype
from gpsiq.scenario import synth_blocks

FS = 2.6e6
RUN = 3                     # blocks of a short unused run
HOLD = 5                    # blocks a slot keeps the satellite it changed to (longer than a thread's four blocks of carry_prefix)
LONG = 300                  # blocks of the long unused run: a whole 256-block chunk of chain_link_scan inside it
GAP = 2                     # plain blocks between two events on one slot
ZERO_SLOPE = 40.0           # Hz per block of the Doppler-through-zero slots (tests/test_eval_edges.py: the map of block B is refused)
MIN_DOPPLER = 2000.0        # Hz: below ~800 Hz a block of 2 048 samples is a slow block, whose map is refused (that is the zero slots' business)


def piece_ends(nblocks, head, max_pieces=8):
    """device_piece_ends of csrc/gpsiq_pieces.h under GPSIQ_PIECE_BLOCKS = head, restated: the first piece has `head` blocks, each
    later one eight times the one before, while what is left is more than one and a half such pieces; head <= 0 or
    2 head > nblocks: one piece.  (tests/piece_plans.cpp pins the planner itself.)"""
    if head <= 0 or 2 * head > nblocks:
        return [nblocks]
    ends, b, size = [head], head, 8 * head
    while nblocks - b > size + size // 2 and len(ends) < max_pieces - 1:
        b += size
        ends.append(b)
        size *= 8
    return ends + [nblocks]


def edge_events(nb, boundaries, reference):
    """Every event a timeline of nb blocks is asked to hold: [(key, lo, hi, what)], lo..hi the blocks of the slot the event owns
    (the run or the stay and the block behind it, where the slot is as it was again), or None where the event does not exist."""
    ev = []

    def add(key, lo, hi, exists=True, **what):
        ev.append((key, lo, hi, what) if exists else (key, None, None, None))

    for B in sorted(set(int(b) for b in boundaries if 0 < b < nb)):
        for off in (-1, 0, 1):
            at = B + off
            add(("change", B, off), at, min(at + HOLD, nb - 1), 1 <= at <= nb - 1, at=at, end=min(at + HOLD, nb))
        lo = max(B - RUN, 0)
        add(("unused_end", B), lo, B, run=(lo, B))                                   # the run ends at B - 1, block B seeds again
        hi = min(B + RUN, nb)
        add(("unused_start", B), B - 1, min(hi, nb - 1), run=(B, hi))
        lo, hi = max(B - 2, 0), min(B + 2, nb)
        add(("unused_straddle", B), lo, min(hi, nb - 1), run=(lo, hi))
    for k in range(1, max(nb // 256, 1) + 1):                                        # [256 k, 256 k + 256) lies inside the run
        lo = 256 * k - (LONG - 256) // 2
        add(("unused_long", k), lo, lo + LONG, lo + LONG < nb, run=(lo, lo + LONG))
    for p in range(nb // 3, nb - RUN - 1, 7):
        add(("comeback", p), p, p + RUN, p >= 1, run=(p, p + RUN))
    add(("unused_block0",), 0, min(RUN, nb - 1), nb > RUN, run=(0, RUN))
    add(("unused_last",), nb - RUN - 1, nb - 1, nb > RUN + 1, run=(nb - RUN, nb))
    add(("change_last",), nb - 1, nb - 1, nb >= 2, at=nb - 1, end=nb)
    if reference:
        # through zero in the first block of a chunk of chain_link_scan, and in the last block of one
        mult = [B for B in sorted(set(int(b) for b in boundaries)) if 0 < B < nb and B % 256 == 0]
        for B in mult[:1] + [m - 1 for m in mult[1:2] or mult[:1]]:
            add(("doppler_zero", B), 0, nb - 1, zero_at=B)
        add(("exact_tie",), 0, nb - 1, tie=True)
    return ev


ONE_OF = ("unused_long", "comeback")           # kinds of which one placed event is enough: the others are alternatives for it


def edge_timeline(nb, nc, boundaries, seed, reference=False, skip=()):
    """synth_blocks(nb, nc, seed) with a fresh carr_phase in every block (only a block that seeds its slot may read it) and the
    events of edge_events() on its slots: first fit, an event never closer than GAP blocks to another one on its slot.  skip: keys
    placed in earlier parts.  Returns (descriptors, record)."""
    d = synth_blocks(nb, nc, seed=seed)
    rng = np.random.default_rng(seed)
    d["carr_phase"] = rng.random((nb, nc))
    d["f_carr"] += np.where(d["f_carr"][0] < 0.0, -MIN_DOPPLER, MIN_DOPPLER)[None, :]
    d["f_code"] = 1.023e6 + d["f_carr"] / 1540.0
    base = d["prn"][0].copy()
    taken = [[] for _ in range(nc)]
    rec = {"placed": [], "deferred": [], "outside": [], "nb": nb, "nc": nc}
    have = set(k[0] for k in skip if k[0] in ONE_OF)
    for key, lo, hi, what in edge_events(nb, boundaries, reference):
        if key in skip or (key[0] in ONE_OF and key[0] in have):
            continue
        if lo is None:
            if key[0] not in ONE_OF:
                rec["outside"].append(key)
            continue
        slot = next((s for s in range(nc) if all(hi + GAP < a or lo - GAP > b for a, b in taken[s])), None)
        if slot is None:
            rec["deferred"].append(key)
            continue
        taken[slot].append((lo, hi))
        have.add(key[0])
        e = dict(key=key, slot=slot, **what)
        if "run" in what:
            d["prn"][what["run"][0]:what["run"][1], slot] = 0
        elif "at" in what:
            d["prn"][what["at"]:what["end"], slot] = 1 + int(base[slot]) % 32
        elif "zero_at" in what:
            d["f_carr"][:, slot] = (np.arange(nb) - what["zero_at"]) * ZERO_SLOPE
            d["f_code"][:, slot] = 1.023e6 + d["f_carr"][:, slot] / 1540.0
        else:
            d["f_carr"][:, slot] = FS / 1024.0                                      # c = 2^-10 exactly: every binade an exact tie
            d["f_code"][:, slot] = 1.023e6 + d["f_carr"][:, slot] / 1540.0
        rec["placed"].append(e)
    # of the alternatives of a ONE_OF kind only a missing one counts
    for kind in ONE_OF:
        if kind not in have and any(k[0] == kind and lo is not None for k, lo, _, _ in edge_events(nb, boundaries, reference)):
            rec["deferred"].append((kind,))
    return d, rec


def edge_timelines(nb, nc, boundaries, seed, reference=False, max_parts=64):
    """edge_timeline() as often as it takes to place every event that exists: [(descriptors, record), ...]"""
    parts, done = [], []
    while True:
        d, rec = edge_timeline(nb, nc, boundaries, seed + len(parts), reference, skip=tuple(done))
        parts.append((d, rec))
        done += [e["key"] for e in rec["placed"]]
        if not rec["deferred"]:
            return parts
        assert rec["placed"] and len(parts) < max_parts, f"events that fit no timeline of {nb} x {nc}: {rec['deferred']}"


def class_timeline(nb, nc=16, seed=5):
    """The launch class (largest code step, most active slots, largest sum of amplitudes: SynthClass) with each maximum in a single
    block where a reduction loses it easily: 13 active slots only in block nb - 1, the last block of a partly filled workgroup
    of pack_raw (nb % 8 != 0); sum of (int)(250 |gain|) > 32767 only in block nb - 19; a code step that needs the half-row kernel
    only in block nb - 10.  Every other block: at most 4 active slots (they move from block to block), small gains.
    Returns (descriptors, {"active": block, "amp": block, "step": block})."""
    assert nc >= 13 and nb % 8 != 0 and nb > 40
    d = synth_blocks(nb, nc, seed=seed)
    d["carr_phase"] = np.random.default_rng(seed).random((nb, nc))
    where = {"active": nb - 1, "amp": nb - 19, "step": nb - 10}
    for b in range(nb):
        keep = [(b // 3 + 5 * j) % nc for j in range(4)]
        if b == where["active"]:
            keep = list(range(1, 14))
        off = np.ones(nc, dtype=bool)
        off[keep] = False
        d["prn"][b, off] = 0
    b = where["amp"]
    d["gain"][b] = np.where(np.arange(nc) % 2, -40.0, 40.0)                         # four active slots: 4 x 10 000 > 32767
    b = where["step"]
    d["f_code"][b] = 2.0e6                                                          # 0.77 chip per sample at 2.6 Msps: 31/63 < step <= 1
    return d, where


def patchy_timeline(nb, nc, seed=3):
    """patchy() of tests/test_gpu_level.py on every channel: code phases a hair short of a chip edge at a whole number of samples
    per chip, where the double code accumulator and the closed form disagree -- GPSIQ_NCO_REFERENCE then has patches.  (The hair
    is 1e-11 chip: a block of 2 048 samples is too short for the accumulator's rounding to cross the 1e-10 of the long blocks.)"""
    d = synth_blocks(nb, nc, seed=seed)
    rng = np.random.default_rng(seed)
    d["code_phase"] = (rng.integers(0, 1023, (nb, nc)) + 1.0 - 1e-11) % 1023.0
    d["f_code"] = FS / 7
    return d


def fixed_reference(orc, d, fs, nsamp, ss):
    """GPSIQ_NCO_FIXED: the oracle's quantiser down the timeline (the carrier carried exactly, seeded again where a slot's satellite
    changes), then the oracle's closed form of every block -> elements [nb][2 nsamp]"""
    q = orc.quantize_blocks(d, fs, nsamp)
    return np.stack([orc.block_fixed(q[b], nsamp, ss) for b in range(d.shape[0])])


def float_reference(orc, d, fs, nsamp, ss):
    """GPSIQ_NCO_REFERENCE: the reference's loop (oracle.block_float) block after block, the carrier handed on here: a slot takes
    its own carr_phase in block 0 or when its satellite is not the one of the block before (an unused slot counts as satellite 0),
    else the state the oracle handed out.  -> (elements [nb][2 nsamp], start states [nb][nc] (0 where the slot is unused), the
    state after the last block as raw doubles: where a slot's last block is unused, that block's carr_phase)"""
    nb, nc = d.shape
    out = np.zeros((nb, 2 * nsamp), dtype=elem_dtype(ss))
    starts = np.zeros((nb, nc))
    state = np.zeros(nc)
    prev = np.zeros(nc, dtype=np.int64)
    for b in range(nb):
        blk = d[b].copy()
        prn = np.maximum(blk["prn"].astype(np.int64), 0)
        cont = (prn > 0) & (prn == prev) & (b > 0)
        blk["carr_phase"][cont] = state[cont]
        starts[b] = np.where(prn > 0, blk["carr_phase"], 0.0)
        out[b], state = orc.block_float(blk, nsamp, fs, ss)
        prev = prn
    return out, starts, state


# ---- the cases of tests/test_gpu_eval_edges.py (tests/test_eval_edges.py checks the same objects on the CPU) --------------------
NB_FIXED, NS_FIXED = 2600, 600
# thread, wave and round edges of carry_prefix; the piece ends of GPSIQ_PIECE_BLOCKS = 1, 3 and 1024; the split points of the continued call
FIXED_BOUNDARIES = tuple(sorted({4, 8, 256, 1024, 2048, 1023} | set(piece_ends(NB_FIXED, 1)[:-1]) | set(piece_ends(NB_FIXED, 3)[:-1])
                                | set(piece_ends(NB_FIXED, 1024)[:-1])))
NB_REFERENCE, NS_REFERENCE = 1100, 2048
REFERENCE_BOUNDARIES = (256, 512, 768, 1024)
SHORT_BLOCKS, NS_SHORT = (1, 2, 7, 8, 9, 255, 256, 257), 2048
SHORT_BOUNDARIES = (4, 8, 256)
NB_CLASS, NS_CLASS = 203, 2048
CLASS_PIECES = (0, 16, 8)                      # one piece; [16, 203]; [8, 72, 203]
NB_PATCHY, NS_PATCHY = 24, 2048
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def fixed_parts(nc):
    return _once(("fixed", nc), lambda: edge_timelines(NB_FIXED, nc, FIXED_BOUNDARIES, 100 + nc))


def reference_parts(nc):
    return _once(("reference", nc), lambda: edge_timelines(NB_REFERENCE, nc, REFERENCE_BOUNDARIES, 200 + nc, reference=True))


def short_parts(nb, nc):
    return _once(("short", nb, nc), lambda: edge_timelines(nb, nc, SHORT_BOUNDARIES, 300 + nb + nc, reference=True))


def first_difference(got, want, d):
    """what an assert says about two renders [nb][2 nsamp] that differ: the first block, its active slots, the elements"""
    rows = np.flatnonzero((got != want).any(axis=1))
    if not len(rows):
        return "equal"
    b = int(rows[0])
    k = np.flatnonzero(got[b] != want[b])
    return (f"{len(rows)} of {len(got)} blocks differ, the first is block {b} ({int((d['prn'][b] > 0).sum())} active slots, prn {d['prn'][b].tolist()}): "
            f"{len(k)} elements, the first at {int(k[0])}: got {got[b][k[:6]].tolist()} want {want[b][k[:6]].tolist()}")
