"""The packed stream formats of include/gpsiq_rows.h ("Packed streams") restated in numpy: pack with clamp and count, and unpack.
    PK4   byte n = (I(n) & 15) | ((Q(n) & 15) << 4)                                  fields -7..7
    PK2   byte m = nib(2m) | (nib(2m+1) << 4),  nib(n) = (I(n) & 3) | ((Q(n) & 3) << 2)   fields -1..1; odd nsamp: high nibble 0
TEST INFRASTRUCTURE: shares no code with the library."""
import numpy as np

PK4, PK2 = 4, 2


def qmax(bits):
    return {PK4: 7, PK2: 1}[bits]


def packed_block_bytes(nsamp, bits):
    if nsamp <= 0 or bits not in (PK4, PK2):
        return 0
    return nsamp if bits == PK4 else (nsamp + 1) // 2


def pack(x, bits):
    """x: integer elements [..., 2 * nsamp], interleaved I,Q -> (uint8 [..., packed_block_bytes], number of elements clamped)"""
    x = np.asarray(x)
    v = x.astype(np.int64)
    q = qmax(bits)
    c = np.clip(v, -q, q)
    clipped = int(np.count_nonzero(c != v))
    nsamp = x.shape[-1] // 2
    i, qq = c[..., 0::2], c[..., 1::2]
    if bits == PK4:
        out = (i & 15) | ((qq & 15) << 4)
    else:
        nib = (i & 3) | ((qq & 3) << 2)
        if nsamp & 1:
            nib = np.concatenate([nib, np.zeros(nib.shape[:-1] + (1,), dtype=nib.dtype)], axis=-1)
        out = nib[..., 0::2] | (nib[..., 1::2] << 4)
    return out.astype(np.uint8), clipped


def unpack(p, nsamp, bits, dtype=np.int8):
    """p: uint8 [..., packed_block_bytes(nsamp)] -> elements [..., 2 * nsamp] of dtype, the fields sign-extended"""
    p = np.asarray(p, dtype=np.uint8).astype(np.int64)
    if bits == PK4:
        f = np.stack([p & 15, p >> 4], axis=-1)
    else:
        f = np.stack([p & 3, (p >> 2) & 3, (p >> 4) & 3, p >> 6], axis=-1)
    f = f.reshape(p.shape[:-1] + (-1,))[..., :2 * nsamp]
    half = 1 << (bits - 1)
    return ((f ^ half) - half).astype(dtype)
