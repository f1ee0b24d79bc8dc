// gpsiq_window_setup.inc -- the state of the sign window walker (gpsiq_signal.h, "The sign window"), included inside a kernel.
// In scope where it is included: q (the channel's descriptor) and n_row (the first sample of the lane's first row).
    const unsigned __int128 T = (unsigned __int128) q.code_frac + (unsigned __int128) q.code_step * (unsigned __int128) n_row;
    const uint64_t A = (uint64_t) q.chip0 + (uint64_t) (T >> GPSIQ_CODE_FRAC_BITS);
    uint64_t fr = (uint64_t) T & kCodeFracMask;
    uint32_t k = (uint32_t) (A % GPSIQ_CA_SEQ_LEN);          // chip inside the period
    const uint64_t ic = q.icode + A / GPSIQ_CA_SEQ_LEN;
    uint32_t bit = (uint32_t) (ic / 20), icur = (uint32_t) (ic % 20);
    uint32_t a5 = (uint32_t) A;                                // only A mod 32 is used
    const uint64_t row_step = q.code_step * 64u;
    const uint32_t d_int = (uint32_t) (row_step >> GPSIQ_CODE_FRAC_BITS);
    const uint64_t d_fr = row_step & kCodeFracMask;
    const uint32_t nav = q.nav_bits;
