// gpsiq_spectrum_geometry.h -- the geometry the spectrum kernels (gpsiq_spectrum_kernels.hip) are compiled for and the planner
// (gpsiq_spectrum_plan.h) cuts its grids by.  These numbers decide device code, so the file is one of the device sources behind
// gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain constants: host and device code include it alike.
#ifndef GPSIQ_SPECTRUM_GEOMETRY_H
#define GPSIQ_SPECTRUM_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kSpecMinFft = 64, kSpecMaxFft = 512, kSpecMaxShift = 40;
constexpr unsigned kSpecMaxGrid = 1u << 20;    // workgroups of a launch at most; spectrum_generic strides over its units past that

// spectrum_generic: a workgroup of min(nfft, 256) threads, a thread owns nfft / threads bins (1 or 2).  A UNIT is a run of up to
// kSpecRun consecutive segments of ONE group: the workgroup sums their cells in registers and adds the sum into power once.
constexpr int kSpecThreads = 256;
constexpr int kSpecRun = 64;
constexpr int kSpecChunk = 32;                 // terms of an int32 partial sum: 32 * 250 * (32768 + 32768) = 524 288 000 < 2^31
constexpr int spectrum_generic_threads(int nfft) { return nfft < kSpecThreads ? nfft : kSpecThreads; }

// spectrum_mfma (int8 input): v_mfma_i32_16x16x64_i8, D = A x B.  A segment is one real sequence of 2N bytes X[e], e = 2 n + c (c = 0:
// I, 1: Q).  A ROW TILE is 16 rows r = 2 kk + comp: component comp (0: i, 1: q) of bin 8 * tile + kk; a COLUMN is a segment, a column
// tile 16 consecutive segments; the k dimension runs over the 2N bytes of the segment, kSpecK per step.
//   A(r, e) = the coefficient of X[e] in Y_comp[k], the window folded in: the same for every segment, tile and workgroup
//   B(e, col) = X[e] of segment col
// A is kept in two balanced base-256 digit planes, A = d0 + 256 d1, in fragment order: lane l's 16 bytes of (plane p, row tile rt,
// k-step t) lie at ((p * row_tiles + rt) * ksteps + t) * 1024 + 16 l.
constexpr int kSpecK = 64, kSpecTileCols = 16, kSpecTileBins = 8, kSpecMaxColTiles = 4;
constexpr int spectrum_row_tiles(int nfft) { return nfft / kSpecTileBins; }
constexpr int spectrum_ksteps(int nfft) { return 2 * nfft / kSpecK; }
constexpr int spectrum_plane_bytes(int nfft) { return spectrum_row_tiles(nfft) * spectrum_ksteps(nfft) * kSpecK * 16; }      // (2N)^2
// A PASS is the `cols` consecutive segments a workgroup stages at once.  The window lies in LDS in chunks of one hop (2 hop bytes),
// each followed by 32 bytes of padding: segment j of the pass starts at chunk j, k-step t of it lies in chunk j + 64 t / (2 hop), and
// the sixteen columns of a tile read 16-byte pieces 2 hop + 32 bytes apart -- 16-byte aligned, and with the 16 bytes a lane group is
// further on, the sixteen lanes a 16-byte LDS read serves together fall on sixteen different 16-byte slots of the 256-byte bank row.
constexpr int spectrum_chunk_stride(int hop) { return 2 * hop + 32; }
constexpr int spectrum_window_bytes(int nfft, int hop, int cols) { return (cols - 1 + nfft / hop) * spectrum_chunk_stride(hop); }
constexpr int kSpecWindowLds = 40960;          // the staged window at most; the workgroup's sums (12 bytes a bin) lie before it
constexpr int spectrum_mfma_cols(int nfft, int hop)
{
    return spectrum_window_bytes(nfft, hop, kSpecMaxColTiles * kSpecTileCols) <= kSpecWindowLds ? kSpecMaxColTiles * kSpecTileCols
                                                                                                : kSpecMaxColTiles * kSpecTileCols / 2;
}
constexpr int spectrum_mfma_sums_bytes(int nfft) { return 16 * nfft; }      // [nfft] uint64 sums, [nfft] uint32 group tags, padded to 16 a bin
constexpr unsigned kSpecMfmaGrid = 2048;       // workgroups the passes are dealt over, each a contiguous range of them

}  // namespace gpsiq
#endif
