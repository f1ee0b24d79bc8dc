// gpsiq_pack_plan.h -- the grid a gpsiq_pack / gpsiq_unpack call (include/gpsiq_rows.h, "Packed streams") takes.  Host code only, and
// pure: no HIP, no environment.  The piece size of gpsiq_generate_batch_packed is stage_piece_blocks (gpsiq_pieces.h), with the
// GPSIQ_PACK_PIECE_BLOCKS override as an argument, read per call by the caller.  tests/pack_plan.cpp pins every plan on the CPU.
// Not a device source: the geometry the kernels are compiled for is gpsiq_pack_geometry.h, the list of kernels that exist is in
// gpsiq_pack_kernels.hip.
#ifndef GPSIQ_PACK_PLAN_H
#define GPSIQ_PACK_PLAN_H

#include <cstddef>
#include <cstdint>

#include "gpsiq_pack_geometry.h"
#include "gpsiq_pieces.h"

namespace gpsiq {

// bytes of one packed block: one byte per complex sample at 4 bits, two samples per byte at 2 bits (0: no such format)
inline size_t packed_block_bytes(int nsamp, int bits)
{
    if (nsamp <= 0) return 0;
    return bits == 4 ? (size_t) nsamp : bits == 2 ? ((size_t) nsamp + 1) / 2 : 0;
}

struct PackPlan {
    bool     launch = false;           // false: no byte to work on, nothing is launched
    unsigned grid = 0, threads = 0;
    uint32_t units = 0;                // units of one block (gpsiq_pack_geometry.h), the last one possibly ragged
    uint32_t tiles = 0;                // workgroup-sized runs of units per block
    uint64_t total = 0;                // tiles * nblocks: workgroup w of the grid takes tiles w, w + grid, ...
};

// unit_bytes: bytes of the block's wide side (pack: source, unpack: destination) one unit covers; side_bytes: that side's length
inline PackPlan plan_units(int nblocks, uint64_t side_bytes, int unit_bytes)
{
    PackPlan p;
    if (nblocks <= 0 || side_bytes == 0 || unit_bytes <= 0) return p;
    const uint64_t units = (side_bytes + (uint64_t) unit_bytes - 1) / (uint64_t) unit_bytes;
    const uint64_t per_tile = (uint64_t) kPackThreads * kPackUnitsPerThread;
    p.launch = true;
    p.threads = kPackThreads;
    p.units = (uint32_t) units;                                    // <= 2^33 / 32: fits
    p.tiles = (uint32_t) ((units + per_tile - 1) / per_tile);
    p.total = (uint64_t) p.tiles * (uint64_t) nblocks;
    p.grid = p.total < kPackMaxGrid ? (unsigned) p.total : kPackMaxGrid;
    return p;
}

inline bool pack_format_ok(int sample_size, int bits) { return (sample_size == 1 || sample_size == 2) && (bits == 4 || bits == 2); }

inline PackPlan plan_pack(int nblocks, int nsamp, int sample_size, int bits)
{
    if (!pack_format_ok(sample_size, bits) || nsamp <= 0) return PackPlan();
    return plan_units(nblocks, (uint64_t) 2 * (uint64_t) nsamp * (uint64_t) sample_size, pack_unit_src_bytes(sample_size, bits));
}

inline PackPlan plan_unpack(int nblocks, int nsamp, int bits, int sample_size)
{
    if (!pack_format_ok(sample_size, bits) || nsamp <= 0) return PackPlan();
    return plan_units(nblocks, (uint64_t) 2 * (uint64_t) nsamp * (uint64_t) sample_size, unpack_unit_dst_bytes(bits, sample_size));
}

// Blocks per piece of gpsiq_generate_batch_packed: the one policy, stage_piece_blocks (gpsiq_pieces.h), under the call's name.  The
// packer takes a piece block by block, not as one span: no sample cap
inline int pack_piece_blocks(int nblocks, size_t src_block_bytes, long override_blocks) { return stage_piece_blocks(nblocks, 0, src_block_bytes, override_blocks); }

}  // namespace gpsiq
#endif
