// gpsiq_window_step.inc -- the sign window walker (gpsiq_signal.h, "The sign window") moves on by one row: less than 32 chips, so
// one period wrap at most, and with it maybe the next data bit.  In scope where it is included: the state of gpsiq_window_setup.inc.
    fr += d_fr;
    const uint32_t adv = d_int + (uint32_t) (fr >> GPSIQ_CODE_FRAC_BITS);
    fr &= kCodeFracMask;
    a5 += adv;
    k += adv;
    if (k >= GPSIQ_CA_SEQ_LEN) {
        k -= GPSIQ_CA_SEQ_LEN;
        if (++icur == 20u) { icur = 0u; ++bit; }
    }
