// gpsiq_exact.h -- what the evaluator of GPSIQ_NCO_REFERENCE (gpsiq_exact.cpp) offers the library's other translation units
// (gpsiq_refwalk.cpp) and the host tests.  Library-internal: none of it is exported.
#ifndef GPSIQ_EXACT_H
#define GPSIQ_EXACT_H

#include "gpsiq_internal.h"

namespace gpsiq {

// One C/A code, generated when a block first has a candidate to look at (most have none).
struct CodeCache {
    int     prn = 0;
    uint8_t ca[GPSIQ_CA_SEQ_LEN];
    const uint8_t *get(int p) { if (p != prn) { ca_code(p, ca); prn = p; } return ca; }
};

inline unsigned nav_bit(const gpsiq_chan_t &ch, long bit)     // the data bit `bit` nav-bit periods after the block's first
{
    const long pos = (long) ch.ibit + bit;
    const long w = (long) ch.iword + pos / 30;
    if (w >= GPSIQ_N_DWRD) return 0;                            // the float loop would run past dwrd[] too; quantize_one rejects it
    return (ch.dwrd[w] >> (29 - (int) (pos % 30))) & 1u;
}

// the order of every patch list the library hands out: (block, sample, slot)
inline bool patch_before(const gpsiq_patch_t &a, const gpsiq_patch_t &b)
{
    if (a.block != b.block) return a.block < b.block;
    if (a.sample != b.sample) return a.sample < b.sample;
    return a.slot < b.slot;
}

// The serial half: the accumulator after the block's nsamp additions of f_carr*delt (gps.c:2821-2826), from `start`.
double chain_block(double f_carr, double delt, int nsamp, double start);

// The parallel half: one channel of one block, given the double the reference's accumulator holds at its start (1.0 included).
// Quantises the descriptor seeded from it (-> q) and appends the samples where the double path takes another LUT entry or
// sign than the closed form (the comment at the definition has the details).
int eval_block(const gpsiq_chan_t &ch, double start, double delt, int nsamp, int block, int slot,
               CodeCache *codes, gpsiq_qchan_t *q, std::vector<gpsiq_patch_t> *out, bool no_drift = false,
               const gpsiq_chan_t *blk = nullptr, int i_in_blk = 0, const uint64_t *seed_override = nullptr);

}  // namespace gpsiq
#endif
