// gpsiq_window_row.inc -- the walker's current row (gpsiq_signal.h, "The sign window"), included inside the kernel's loop over the
// lane's rows: declares S, the signs of the 32 chips from chip k on; window_word(S, a5) is the row's window word.  In scope where it
// is included: the state of gpsiq_window_setup.inc, ext (the staged codes) and c (the channel).
    // 32 chips starting at chip k of the (wrap-extended) code
    const uint32_t lo = ext[c][k >> 5], hi = ext[c][(k >> 5) + 1];
    uint32_t S = __builtin_amdgcn_alignbit(hi, lo, k & 31u);
    // chips at window positions >= 1023-k belong to the next code period
    const uint32_t to_wrap = GPSIQ_CA_SEQ_LEN - k;
    const uint32_t next_mask = to_wrap < 32u ? (0xffffffffu << to_wrap) : 0u;
    const uint32_t bit_next = icur == 19u ? bit + 1u : bit;
    const uint32_t d0 = 0u - ((nav >> (bit & 31u)) & 1u);
    const uint32_t d1 = 0u - ((nav >> (bit_next & 31u)) & 1u);
    S ^= (d0 & ~next_mask) ^ (d1 & next_mask);
