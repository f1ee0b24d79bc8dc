"""The timelines of tests/test_gpu_desc_memory.py: gpsiq_generate_batch with its descriptors in page-locked and in device memory, on
every path of the call.  Each timeline is built for what the HOST path reads from ch beyond the bulk rows -- block 0 (the
continuation test), the block behind a piece's end (does the slot keep its satellite), the last block (the phase handed out for a
slot that ends unused), the row a refused descriptor's message is written from.  Pure numpy on gpsiq.scenario.synth_blocks: nothing
here calls libgpsiq or needs a GPU.  tests/test_desc_memory_cases.py holds the table to what its names say.  TEST INFRASTRUCTURE."""
import numpy as np

from gpsiq.scenario import synth_blocks

FS = 2.6e6
NSAMP = 13000                   # 5 ms: not a multiple of 64, and a block of 26 000 / 52 000 bytes is a multiple of 16 (rendered where it lies)

# `edges`: which slot holds what
NB_EDGES, NC_EDGES = 40, 6
SLOT_CHANGES, CHANGE_AT = 0, (8, 16)            # another satellite from block 8, a third one from block 16
SLOT_LATE, LATE_START = 1, 3                    # unused in blocks 0..2, then starts
SLOT_REFUSED, REFUSED_AT = 2, 30                # plain in `edges`; `refused` has f_code = 0 there
SLOT_ENDS_UNUSED = 3                            # unused in the last block only
SLOT_ZERO, ZERO_AT, ZERO_SLOPE = 4, 20, 1.5     # Doppler through zero: negative before block 20, 0 in it, positive after (Hz per block)
CUT = 20                                        # where the continuation test cuts `edges` into two calls
# the reference model's threshold (device_path_wanted, csrc/gpsiq_evaldev.cpp): 48 blocks
NB_SHORT_REF, NB_LONG_REF, NC_REF = 47, 48, 16


def _fresh_phases(d, seed):
    """a carr_phase of its own in every block: only a block that seeds its slot may read it, and one that does must read this one"""
    d["carr_phase"] = np.random.default_rng(seed).random(d.shape)
    return d


def edges():
    d = _fresh_phases(synth_blocks(NB_EDGES, NC_EDGES, seed=611), 611)
    d["prn"][CHANGE_AT[0]:CHANGE_AT[1], SLOT_CHANGES] = 11
    d["prn"][CHANGE_AT[1]:, SLOT_CHANGES] = 12
    d["prn"][:LATE_START, SLOT_LATE] = 0
    d["prn"][-1, SLOT_ENDS_UNUSED] = 0
    d["f_carr"][:, SLOT_ZERO] = (np.arange(NB_EDGES) - ZERO_AT) * ZERO_SLOPE
    d["f_code"][:, SLOT_ZERO] = 1.023e6 + d["f_carr"][:, SLOT_ZERO] / 1540.0
    return d


def one():
    return _fresh_phases(synth_blocks(1, 3, seed=612), 612)


def _ref_timeline(nb, seed):
    """sixteen channels; slot 2 changes satellite half-way, slot 5 ends unused"""
    d = _fresh_phases(synth_blocks(nb, NC_REF, seed=seed), seed)
    d["prn"][nb // 2:, 2] = 20
    d["prn"][-1, 5] = 0
    return d


def refused():
    d = edges()
    d["f_code"][REFUSED_AT, SLOT_REFUSED] = 0.0
    return d


_MAKE = {"edges": edges, "one": one, "short-ref": lambda: _ref_timeline(NB_SHORT_REF, 613), "long-ref": lambda: _ref_timeline(NB_LONG_REF, 614),
         "refused": refused}
NAMES = tuple(_MAKE)
_cache = {}


def timeline(name):
    """the descriptors of a case, built once; read-only (a test that changes rows takes a copy)"""
    if name not in _cache:
        d = _MAKE[name]()
        d.setflags(write=False)
        _cache[name] = d
    return _cache[name]
