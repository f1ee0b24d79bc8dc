// gpsiq_pack_geometry.h -- the geometry the pack / unpack kernels (gpsiq_pack_kernels.hip) are compiled for and the planner
// (gpsiq_pack_plan.h) cuts its grids by.  These numbers decide device code, so the file is one of the device sources behind
// gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain constants: host and device code include it alike.
#ifndef GPSIQ_PACK_GEOMETRY_H
#define GPSIQ_PACK_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kPackThreads = 256;              // four waves per workgroup, every kernel
constexpr int kPackUnitsPerThread = 4;         // units a thread works through per tile, kPackThreads apart (loads of a step contiguous over the workgroup)
constexpr unsigned kPackMaxGrid = 1u << 20;    // workgroups of a launch at most; the kernels stride over tiles past that

// A UNIT is what one lane loads, converts and stores in one go.
//   pack:   kPackLoads(fmt, bits) 16-byte loads of consecutive source bytes -> ONE store of 16 bytes (8 for int16 -> 2 bit)
//   unpack: ONE 16-byte load of packed bytes -> 32 .. 128 bytes of elements in 16-byte stores
// Source bytes of a pack unit / packed bytes it makes
constexpr int pack_unit_loads(int sample_size, int bits) { return sample_size == 1 && bits == 4 ? 2 : 4; }
constexpr int pack_unit_src_bytes(int sample_size, int bits) { return 16 * pack_unit_loads(sample_size, bits); }
constexpr int pack_unit_dst_bytes(int sample_size, int bits) { return pack_unit_src_bytes(sample_size, bits) / sample_size * bits / 8; }
// Packed bytes of an unpack unit / element bytes it makes
constexpr int unpack_unit_src_bytes() { return 16; }
constexpr int unpack_unit_dst_bytes(int bits, int sample_size) { return 16 * 8 / bits * sample_size; }

}  // namespace gpsiq
#endif
