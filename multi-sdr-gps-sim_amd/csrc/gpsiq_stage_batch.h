// gpsiq_stage_batch.h -- the piece loop of the staged batch calls gpsiq_generate_batch_packed / _filtered / _mixed / _resampled / _agc
// (include/gpsiq_rows.h) and the staging ring the device context holds for them (gpsiq_ctx.h: the member `ring`).  Host code.  The
// loop is in gpsiq_stage_batch.cpp; the piece size (stage_piece_blocks) and the phase hand-over (piece_rows) are pure and in
// gpsiq_pieces.h.  A stage's own share of such a call -- checks, plan, tables, kernels -- stays in gpsiq_<stage>.cpp.
//
// Piece p: gpsiq_generate_batch renders its blocks back to back into d_render[p & 1], `lead` bytes in (synchronous); the stage
// queues its work on stage_stream; the result crosses to the host on copy_stream behind the event staged[p & 1] -- while the calling
// thread is already in the render of piece p + 1, which uses the other pair.  Piece p + 2 takes pair p & 1 again once copied[p & 1]
// of piece p has been reached, which lies behind staged[p & 1] and with it behind everything the stage queued for piece p.
// Where the stage reads history (hist > 0: the last `hist` bytes in front of a span, lead >= hist), it crosses inside the staging:
// behind the stage's work of piece p, on stage_stream, the last `hist` bytes of [lead region | piece p] are copied to the end of the
// other pair's lead region -- right for a piece shorter than the history too, whose own lead region then supplies the rest.  The
// first piece's is the caller's to fill (zeros), per call: the ring holds whatever the call before left, of whichever stage.
// The carrier phases cross on the host (piece_rows); gpsiq_generate_batch numbers the noise blocks on from call to call.
// On every path the call ends with both streams drained: nothing of it still reads the staging or writes dst when it returns, and
// the next call on the context -- calls on a context are serial -- finds the ring idle.
#ifndef GPSIQ_STAGE_BATCH_H
#define GPSIQ_STAGE_BATCH_H

#include <functional>
#include <vector>

#include "gpsiq_internal.h"
#include "gpsiq_own.h"

namespace gpsiq {

// two rendered and two output staging buffers taken in turn (a stage that works in place uses the rendered pair alone), a stream for
// the stage's work, one for the copies, per pair the events "staged" and "copied", and the descriptors of a piece with the carrier
// phases handed over in its first block
struct PieceRing {
    DevBuf<uint8_t>           d_render[2], d_out[2];                                      // bytes
    Stream                    stage_stream, copy_stream;
    Event                     staged[2], copied[2];
    std::vector<gpsiq_chan_t> row;
    int reserve(size_t render_bytes, size_t out_bytes);         // first use + room for one call's pieces (out_bytes 0: in place)
};

// (streams and events on first use; the staging pairs grow together, rendered side first)
inline int PieceRing::reserve(size_t render_bytes, size_t out_bytes)
{
    HIP_TRY(stage_stream.ensure());
    HIP_TRY(copy_stream.ensure());
    for (auto &e : staged) HIP_TRY(e.ensure());
    for (auto &e : copied) HIP_TRY(e.ensure());
    HIP_TRY(reserve_together(render_bytes, render_bytes + render_bytes / 4 + 256, d_render[0], d_render[1]));
    HIP_TRY(reserve_together(out_bytes, out_bytes + out_bytes / 4 + 256, d_out[0], d_out[1]));
    return GPSIQ_OK;
}

// what a stage tells the loop
struct StageBatch {
    const char *label;                 // "filtered batch": the error texts
    int         sample_size;           // of the rendered stream
    size_t      lead, hist;            // bytes in front of the rendered blocks in d_render[]; the history handed from pair to pair
    int         piece;                 // blocks per piece
    const unsigned long long *d_count; // the stage's counter of clamped elements, zeroed by the stage before the first piece ...
    unsigned long long       *h_count; // ... and its page-locked twin, read once behind the last piece
    // 64-bit words that come back from d_count to h_count behind the last piece.  The first is the counter; a stage with more to
    // fetch (gpsiq_generate_batch_agc: a second counter and the state it kept on the device) lays it out behind that word
    size_t      count_words = 1;
};

// a piece as the stage sees it: blocks [b0, b0 + nb) of the call, rendered back to back at span = d_render[pair] + lead
struct Piece { int p, b0, nb, pair; uint8_t *span; };

// what of a piece crosses to the host: `rows` rows of `width` bytes (rows 0: nothing)
struct PieceCopy {
    const void *src = nullptr; size_t src_pitch = 0, width = 0, rows = 0;
    void       *dst = nullptr; size_t dst_pitch = 0;
};

// queues the stage's work for a piece on the ring's stage_stream and says what to copy; called for nsamp > 0 only
using StageQueue = std::function<int(const Piece &, PieceCopy *)>;

}  // namespace gpsiq

// gpsiq_stage_batch.cpp.  begin: the call's entry, before anything is queued -- ch is host memory (the pieces' first rows are
// rewritten on the host; call: the call's name, for gpsiq_rows_kind's text), the context's device is current, the ring has room
// for a piece (out_bytes 0: the stage works in place).  run: the pieces, the counter's way back and the drain.  rc: what the stage's
// own prologue on stage_stream returned -- not GPSIQ_OK: the call has failed already, nothing more is queued, the streams are
// drained and its error text stands.  carr[GPSIQ_MAX_CHAN]: zeros in, the phases the last piece handed out.  *count: the counter
// (0 where nsamp == 0: it was never written).
int gpsiq_stage_batch_begin(gpsiq_ctx *c, const char *call, const gpsiq_chan_t *ch, size_t render_bytes, size_t out_bytes);
int gpsiq_stage_batch_run(gpsiq_ctx *c, const gpsiq::StageBatch &st, int rc, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs,
                          const gpsiq::StageQueue &queue, double *carr, uint64_t *count);
#endif
