// gpsiq_stage_batch.cpp -- the piece loop of gpsiq_generate_batch_packed / _filtered / _mixed / _resampled / _agc (gpsiq_stage_batch.h says
// what it does and what a stage gives it): the one place that holds pair reuse, the history's way from pair to pair, stream order,
// the drain and the counter that is read only if it was written.  Host code: nothing here decides device code, so the file is not
// one of the device sources behind gpsiq_kernels_id().
#include "gpsiq_ctx.h"
#include "gpsiq_stage_batch.h"

using namespace gpsiq;

int gpsiq_stage_batch_begin(gpsiq_ctx *c, const char *call, const gpsiq_chan_t *ch, size_t render_bytes, size_t out_bytes)
{
    if (int rc = gpsiq_rows_kind(c, ch, call, nullptr)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return c->ring.reserve(render_bytes, out_bytes);
}

int gpsiq_stage_batch_run(gpsiq_ctx *c, const StageBatch &st, int rc, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs,
                          const StageQueue &queue, double *carr, uint64_t *count)
{
    PieceRing &r = c->ring;
    const hipStream_t ss = r.stage_stream.get(), cs = r.copy_stream.get();
    const size_t blk_bytes = block_bytes(nsamp, st.sample_size);
    const int npieces = (nblocks + st.piece - 1) / st.piece;
    for (int p = 0; p < npieces && rc == GPSIQ_OK; ++p) {
        const int b0 = p * st.piece, nb = nblocks - b0 < st.piece ? nblocks - b0 : st.piece, pair = p & 1;
        const gpsiq_chan_t *rows = piece_rows(ch, b0, nb, nchan, carr, &r.row);
        if (p >= 2) {                                                 // the pair's last user: piece p - 2
            const hipError_t e = hipEventSynchronize(r.copied[pair].get());
            if (e != hipSuccess) { rc = fail(GPSIQ_E_DEVICE, "%s: %s", st.label, hipGetErrorString(e)); break; }
        }
        uint8_t *span = r.d_render[pair].get() + st.lead;
        rc = gpsiq_generate_batch(c, rows, nb, nchan, nsamp, fs, st.sample_size, span, 1, carr);
        if (rc != GPSIQ_OK) break;
        if (nsamp == 0) continue;
        PieceCopy cp;
        rc = queue(Piece{p, b0, nb, pair, span}, &cp);
        if (rc != GPSIQ_OK) break;
        hipError_t e = hipSuccess;
        if (st.hist && p + 1 < npieces)                               // the next piece's history
            e = hipMemcpyAsync(r.d_render[pair ^ 1].get() + st.lead - st.hist, span + blk_bytes * (size_t) nb - st.hist, st.hist, hipMemcpyDeviceToDevice, ss);
        if (e == hipSuccess) e = hipEventRecord(r.staged[pair].get(), ss);
        if (e == hipSuccess) e = hipStreamWaitEvent(cs, r.staged[pair].get(), 0);
        if (e == hipSuccess && cp.rows == 1) e = hipMemcpyAsync(cp.dst, cp.src, cp.width, hipMemcpyDeviceToHost, cs);      // one row has no pitch
        if (e == hipSuccess && cp.rows > 1) e = hipMemcpy2DAsync(cp.dst, cp.dst_pitch, cp.src, cp.src_pitch, cp.width, cp.rows, hipMemcpyDeviceToHost, cs);
        if (e == hipSuccess) e = hipEventRecord(r.copied[pair].get(), cs);
        if (e != hipSuccess) rc = fail(GPSIQ_E_DEVICE, "%s piece: %s", st.label, hipGetErrorString(e));
    }
    if (rc == GPSIQ_OK && nsamp) {                                    // the pieces' sum, behind the last piece's work
        const hipError_t e = hipMemcpyAsync(st.h_count, st.d_count, sizeof(unsigned long long) * st.count_words, hipMemcpyDeviceToHost, ss);
        if (e != hipSuccess) rc = fail(GPSIQ_E_DEVICE, "%s count: %s", st.label, hipGetErrorString(e));
    }
    // nothing of the call may still read the staging or write dst when it returns, on any path
    hipError_t e = hipStreamSynchronize(ss);
    const hipError_t d = hipStreamSynchronize(cs);
    if (e == hipSuccess) e = d;
    if (rc != GPSIQ_OK) return rc;                                    // the call has failed already: its error text stands
    if (e != hipSuccess) return fail(GPSIQ_E_DEVICE, "%s: %s", st.label, hipGetErrorString(e));
    *count = nsamp ? (uint64_t) st.h_count[0] : 0;
    return GPSIQ_OK;
}
