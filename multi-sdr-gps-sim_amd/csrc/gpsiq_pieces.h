// gpsiq_pieces.h -- how the batch calls of libgpsiq cut a timeline into pieces.  Host code only, and pure: the measured kernel
// rate and the host thread count come in as arguments (callers pass rate_kernel() and host_threads()), and so does the
// GPSIQ_PIECE_BLOCKS override, which piece_blocks_env() alone reads (per call: A/B in one process).  tests/piece_plans.cpp pins
// every plan on the CPU.
//
// What GPSIQ_PIECE_BLOCKS = n means on each path (unset: the plans below):
//   d2h_chunk_blocks    fixed model, host path, host destination: blocks per piece; n <= 0: one kernel, then one copy
//   batch_piece_blocks  fixed model, long batch into device memory: the nominal piece (the first one is an eighth of it);
//                       n <= 0 or 2 n > nblocks: one piece, and the call takes the host path
//   ref_chunk_blocks    reference model, host walk: the chunk of piece_ends; n <= 0 or n >= nblocks: one piece
//   device_piece_ends   device evaluation: blocks of the first piece, each later one eight times the one before;
//                       n <= 0 or 2 n > nblocks: one piece
// The staged batch calls (gpsiq_stage_batch.h) have an override each, GPSIQ_PACK_ / FILTER_ / MIX_ / RESAMPLE_PIECE_BLOCKS = n:
//   stage_piece_blocks  blocks per piece, as far as the call goes and a piece's samples fit an int; n <= 0: the plan below
// This header also holds what the pieces of those calls hand each other on the host: piece_rows.
#ifndef GPSIQ_PIECES_H
#define GPSIQ_PIECES_H

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <vector>

#include "../../include/gpsiq.h"             // gpsiq_chan_t: piece_rows

namespace gpsiq {

// Block geometry: the bytes of one rendered block (nsamp complex elements of sample_size bytes per component), and between blocks
// where the library lays them out itself (16-byte rows)
inline size_t block_bytes(int nsamp, int sample_size) { return (size_t) 2 * (size_t) nsamp * (size_t) sample_size; }
inline size_t block_stride(int nsamp, int sample_size) { return (block_bytes(nsamp, sample_size) + 15) & ~(size_t) 15; }

inline std::optional<long> piece_blocks_env()
{
    if (const char *e = std::getenv("GPSIQ_PIECE_BLOCKS")) return std::atol(e);
    return std::nullopt;
}

// Blocks per piece of a host-destination batch: the kernel of piece k+1 runs while piece k crosses PCIe (two copy streams, so
// consecutive copies queue back to back).  0 = one kernel, then one copy (the round-1 behaviour, kept for A/B measurements).
inline int d2h_chunk_blocks(size_t stride, std::optional<long> ov)
{
    if (ov) return *ov > 0 ? (int) *ov : 0;
    const size_t target = (size_t) 32 << 20;                 // ~32 MiB per piece: >= 0.5 ms on the link, a few hundred workgroups
    const size_t n = (target + stride - 1) / stride;
    return (int) (n < 8 ? 8 : n);
}

// Blocks per piece of a long device-destination batch in the fixed-point model: ~1 ms of kernel, a few hundred microseconds of
// host work per piece.  nblocks: one piece.
inline int batch_piece_blocks(int nblocks, int nsamp, std::optional<long> ov)
{
    long n = nsamp > 0 ? ((long) 1024 * 260000) / nsamp : 1024;
    if (n > 1024) n = 1024;
    if (n < 32) n = 32;
    if (ov) n = (int) *ov;
    return n > 0 && 2 * n <= nblocks ? (int) n : nblocks;            // fewer than two pieces' worth: one piece
}

// The chunk of a GPSIQ_NCO_REFERENCE batch walked on the host.  A piece costs the renderer ~0.1-0.2 ms (validate + compact +
// upload + launch) whatever its size and nothing on the walkers' side, and should be enough samples for a launch that fills the
// chip: 256 blocks at 2.6 Msps (1.6 ms of walking, 0.2 ms of kernel), fewer at higher rates where a block is more device work
// (25 Msps: 26 blocks = 66 M samples).
inline int ref_chunk_blocks(int nblocks, int nsamp, std::optional<long> ov)
{
    long n = nsamp > 0 ? ((long) 256 * 260000) / nsamp : 256;
    if (n > 256) n = 256;
    if (n < 16) n = 16;
    if (ov) n = (int) *ov;
    return n > 0 && n < nblocks ? (int) n : nblocks;
}

// Piece boundaries of a range of `n` blocks starting at block `first` of the walk, `chunk` blocks each.  Nothing renders before
// the first piece is through all channels: half a chunk.  After that it depends on which side is the slower one.  HOST-bound
// (the rule at 2.6 - 10 Msps): a chunk, then two chunks each, and a chunk and half a chunk again at the end -- the last piece's
// kernel is all that is left after the host has finished.  KERNEL-bound (25 Msps: a block is 6.7 us of device work against
// ~3 us of host work per thread): every launch costs ~30 us beyond its share of one big launch (a 26-block piece is a single
// round of workgroups: 215 us measured against 183 us), so as few pieces as the host can keep ahead of -- each 2.2 x the one
// before (the host has piece k+1 ready before the kernel of piece k ends), no small tail.
inline void piece_ends(int first, int n, int chunk, std::vector<int> *ends, bool kernel_bound = false)
{
    const int half = chunk > 1 ? chunk / 2 : 1;
    if (n <= 4 * chunk) {
        for (int b = chunk; b < n; b += chunk) ends->push_back(first + b);
        ends->push_back(first + n);
        return;
    }
    if (kernel_bound) {
        const int growth = 220;                           // per cent
        int b = 0, size = half;
        while (n - b > size + half) {                // what is left after this piece is worth a piece of its own
            b += size;
            ends->push_back(first + b);
            size = (int) (((long) size * growth + 50) / 100);
            if (size > 16 * chunk) size = 16 * chunk;
        }
        ends->push_back(first + n);
        return;
    }
    const int tail0 = n - chunk - half;               // the last two pieces: a chunk, half a chunk
    int b = half;
    ends->push_back(first + b);
    b += chunk;
    ends->push_back(first + b);
    while (tail0 - b >= 3 * chunk) { b += 2 * chunk; ends->push_back(first + b); }     // what is left (chunk .. 3 chunks) is one piece
    if (tail0 > b) ends->push_back(first + tail0);
    ends->push_back(first + n - half);
    ends->push_back(first + n);
}

// Whether a GPSIQ_NCO_REFERENCE batch is clearly kernel-bound, from the rates measured on MI355X + EPYC 9575F (DESIGN.md section
// 2): the kernel at rate_kernel channel-samples/s, the host at 2.5 us + 0.8 us per 10^6 samples per block and channel on each of
// its threads (2.7 us at 2.6 Msps, 4.5 us at 25 Msps, in the call).  At 25 Msps on sixteen threads the two sides are within 1.5 x
// of each other and the symmetric ramp measured better (1.77 against 1.91 ms per 200 blocks): only a clear case takes the few
// growing pieces.
inline bool ref_kernel_bound(int nsamp, int nchan, double rate_kernel, int host_threads)
{
    const int threads = host_threads < nchan ? host_threads : nchan;
    const double t_kernel = (double) nsamp * (double) nchan / rate_kernel;
    const double t_host = (double) nchan * (2.5e-6 + 0.8e-12 * (double) nsamp) / (double) (threads > 0 ? threads : 1);
    return t_kernel > 2.0 * t_host;
}

// The head of a GPSIQ_NCO_REFERENCE batch whose carrier chain (level 1) runs on the device in two launches: the first piece end
// of `ends` worth ~0.4 ms of synthesis (the second launch's latency + its first piece's evaluation); a bigger head measured
// better than a smaller one (2.35 ms per call at 900 blocks, 2.49 at 256, 2.55 at 128).  nblocks: one launch.
inline int ref_head(const std::vector<int> &ends, int nblocks, int nsamp, int nchan, double rate_kernel)
{
    int head = nblocks;
    const double t_block = (double) nsamp * (double) nchan / rate_kernel;
    const int want = (int) (0.4e-3 / t_block) + 1;
    if (want > 0 && 2 * want < nblocks)
        for (size_t k = 0; k < ends.size(); ++k)
            if (ends[k] >= want) { head = ends[k]; break; }
    if (2 * head > nblocks) head = nblocks;                // what is left would not be worth a launch of its own
    return head;
}

// Piece boundaries of the device evaluation.  A piece's synthesis waits for its own descriptors only (pack, estimate, quantise),
// so pieces exist to start the first synthesis early and to stage piece k+1 under the synthesis of piece k; every further piece
// costs a launch ramp (~0.05 ms).  Descriptors the device reads where they lie stage in microseconds: one piece in the fixed-point
// model, a short head in GPSIQ_NCO_REFERENCE (chain_prepare is 16 workgroups walking the timeline: 25 us per 1 000 blocks).
// Descriptors in host memory (pageable, or page-locked: they cross PCIe too) are packed by the pool at ~14 x the synthesis rate
// (16 threads; 2 x with two): a head worth 0.35 ms of synthesis, so that the pack of what follows hides under it, then pieces
// eight times the one before (measured, 2.6 Msps: 2 000 blocks fixed model 1.56 ms per call against 1.74 with a 0.1 ms head,
// reference model 1.85 against 2.06).  At most max_pieces pieces.
inline void device_piece_ends(int nblocks, int nsamp, int nchan, bool host_rows, bool reference, double rate_kernel,
                              std::optional<long> ov, int max_pieces, std::vector<int> *ends)
{
    const double t_block = (double) nsamp * (double) nchan / rate_kernel;
    long head = (long) ((host_rows ? 0.35e-3 : 0.15e-3) / (t_block > 0.0 ? t_block : 1e-6)) + 1;
    if (head < 16) head = 16;
    if (!host_rows && !reference) head = 0;
    if (ov) head = *ov;
    const long growth = 8;
    if (head <= 0 || 2 * head > nblocks) { ends->push_back(nblocks); return; }
    long b = head, size = growth * head;
    ends->push_back((int) b);
    while (nblocks - b > size + size / 2 && (int) ends->size() < max_pieces - 1) {
        b += size;
        ends->push_back((int) b);
        size *= growth;
    }
    ends->push_back(nblocks);
}

// Blocks per piece of a staged batch call (gpsiq_generate_batch_packed / _filtered / _mixed / _resampled): ~32 MiB of rendered
// stream per piece (the policy of d2h_chunk_blocks: >= 0.5 ms of rendering for the copy of the piece before to hide under), at
// least one block, at most the call's; override_blocks > 0 (the stage's GPSIQ_*_PIECE_BLOCKS) replaces the default.  Where a piece
// is one span of its stage (nsamp >= 1: filter, mixer, resampler) its samples fit an int, whatever was asked for; nsamp = 0 (the
// packer, which works block by block): no such cap.
inline int stage_piece_blocks(int nblocks, int nsamp, size_t block_bytes, long override_blocks)
{
    if (nblocks <= 0) return 0;
    long n;
    if (override_blocks > 0) n = override_blocks;
    else {
        const size_t target = (size_t) 32 << 20;
        const size_t q = block_bytes ? (target + block_bytes - 1) / block_bytes : (size_t) nblocks;
        n = q > (size_t) nblocks ? (long) nblocks : (long) q;
    }
    const long most = nsamp > 0 ? (long) (INT32_MAX / nsamp) : (long) nblocks;
    if (n > most) n = most;
    if (n < 1) n = 1;
    return n > nblocks ? nblocks : (int) n;
}

// The descriptors the piece of blocks [b0, b0 + nb) of such a call is rendered from.  The pieces are chained as a host chains calls
// (host/gpsiq_runahead.c): the first piece takes the caller's rows as they lie; a later piece's first block carries, in every slot
// that keeps its satellite across the edge, the phase the piece before handed out (carr), and a slot whose satellite changes there
// seeds itself from its own carr_phase, as it does inside one call.  Every other row is the caller's.  row: the copy's home.
inline const gpsiq_chan_t *piece_rows(const gpsiq_chan_t *ch, int b0, int nb, int nchan, const double *carr, std::vector<gpsiq_chan_t> *row)
{
    const gpsiq_chan_t *rows = ch + (size_t) b0 * nchan;
    if (b0 == 0) return rows;
    row->assign(rows, rows + (size_t) nb * nchan);
    for (int i = 0; i < nchan; ++i)
        if (rows[i].prn > 0 && rows[i].prn == ch[(size_t) (b0 - 1) * nchan + i].prn) (*row)[i].carr_phase = carr[i];
    return row->data();
}

}  // namespace gpsiq
#endif
