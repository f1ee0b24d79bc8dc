// gpsiq_tile_body.inc -- the body of the tile kernels (gpsiq_kernels.hip: synth_tile, synth_tile_noise and synth_tile_level), included
// inside each.
// Textual inclusion rather than a shared device function: inlining a function (its parameters, its early return) gives the
// compiler another IR to schedule, and the noise-off kernels must stay the code they were.  In scope where it is included:
// the kernel parameters, FMT NCH ROWS H FAST WAVES BOTH, NOISE with ntab / nseed / nblock0 (the receiver noise), and LEVEL with
// lmult / lqmax (the output level stage, include/gpsiq_rows.h; LEVEL kernels are NOISE kernels).
    constexpr int kLutEntries = BOTH ? 1024 : 512;
    // the output level works on the whole 16-bit sums: both formats then accumulate with the int16 table layout (the int8 core's
    // 12-bit fields hold the sums modulo 2^12 only)
    constexpr int LFMT = LEVEL ? GPSIQ_SC16 : FMT;
    static_assert(!LEVEL || (NOISE && !BOTH), "the level stage follows the noise in the noise kernels");
    constexpr int kThreads = WAVES * 64;
    __shared__ uint32_t lut[NCH][kLutEntries];
    __shared__ uint32_t ext[NCH][kPrnExtWords];
    __shared__ uint32_t win[WAVES][ROWS * H][NCH];      // one window per (row or half row, channel)
    __shared__ gpsiq_qchan_t qs[NCH];
    static_assert(H == 1 || H == 2, "one window per row or per half row");
    static_assert(!BOTH || FAST, "the both-polarity table is a form of the plain-add core");
    static_assert(kLutEntries % kThreads == 0 || kThreads % kLutEntries == 0, "LUT build: whole passes");
    constexpr int kSpan = 64 / H;                        // samples per window

    const int tid = threadIdx.x;
    // workgroups [0, big_wgs) give every wave `wave_rows` consecutive rows (several chunks of
    // ROWS rows, the last one possibly partial) of blocks [0, big_blocks); the rest of the grid
    // covers the last blocks with one-chunk workgroups, so that what is still running when the
    // grid drains is short (workgroups are dispatched in id order)
    int blk, tile;
    if ((int) blockIdx.x < big_wgs) {
        blk = blockIdx.x / tiles_per_block; tile = blockIdx.x % tiles_per_block;
    } else {
        const int r = (int) blockIdx.x - big_wgs;
        blk = big_blocks + r / tiles_small; tile = r % tiles_small;
        wave_rows = ROWS;
    }
    const gpsiq_qchan_t *q_blk = desc + (size_t) (block0 + blk) * nchan;
    const int nq = nchan < NCH ? nchan : NCH;
    for (int i = tid; i < NCH * 12; i += kThreads)
        reinterpret_cast<uint32_t *>(qs)[i] = i < nq * 12 ? reinterpret_cast<const uint32_t *>(q_blk)[i] : 0u;
    __syncthreads();
    for (int e = tid; e < kLutEntries; e += kThreads) {
        // entry e of every channel (one pass: a thread per entry); unused slots have gain 0.0 -> entry 0.
        // BOTH: the upper half is the table half a cycle on, i.e. the negated entries
        const int k = BOTH ? (e + ((e >> 9) << 8)) & 511 : e;
        const double sk = (double) dev_sin512(tab->quarter_wave, k);
        const double ck = (double) dev_sin512(tab->quarter_wave, k + 128);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const double g = qs[c].gain;
            const int ts = (int) (sk * g), tc = (int) (ck * g);   // gps.c:2781-2782
            // int8 output keeps bits 4..11 of each 16-bit sum (gps.c:2845): with the entries
            // pre-shifted by 4 (still modulo 2^16) those bits are bytes 1 and 3 of the packed sum
            constexpr int kPre = LFMT == GPSIQ_SC08 ? 4 : 0;
            if (FAST && LFMT == GPSIQ_SC08)
                // the int8 output keeps bits 4..11 of I and Q only: 12-bit fields, I at bits 4..15 (its
                // carries spill into bits 16..19, 16 channels x 12 bits), Q at bits 20..31; the output
                // bytes are bytes 1 and 3 of the plain 32-bit sum, for any gain
                lut[c][e] = (((uint32_t) tc & 0xfffu) << 4) | ((uint32_t) ts << 20);
            else if (FAST)
                // one integer; |tc|, |ts| <= 32767 here.  Slot 0 also carries the +0x8000 that keeps
                // I + 32768 >= 0 in the sum (so a negative I never borrows from the Q half)
                lut[c][e] = (uint32_t) (tc + ts * 65536) + (c == 0 ? 0x8000u : 0u);
            else      lut[c][e] = (((uint32_t) tc << kPre) & 0xffffu) | ((uint32_t) ts << (16 + kPre));
        }
    }
    for (int e = tid; e < NCH * kPrnExtWords; e += kThreads) {
        const int c = e / kPrnExtWords, w = e % kPrnExtWords;
        ext[c][w] = qs[c].prn ? tab->prn_ext[qs[c].prn - 1][w] : 0u;
    }
    [[maybe_unused]] const noise::Entry *nz = nullptr;
    if constexpr (NOISE) {
        __shared__ noise::Entry nz_s[noise::kTabEntries];
        for (int e = tid; e < noise::kTabEntries; e += kThreads) nz_s[e] = ntab[e];
        nz = nz_s;
    }
    __syncthreads();
    uint8_t *blk_dst = dst + (size_t) blk * block_stride;

    const int wave = tid >> 6, lane = tid & 63;
    const uint32_t wave_samples = (uint32_t) wave_rows * 64u;
    const uint32_t n_wave = ((uint32_t) tile * WAVES + (uint32_t) wave) * wave_samples;
    if (n_wave >= (uint32_t) nsamp) return;             // whole wave past the block end
    [[maybe_unused]] uint64_t nx = 0;                   // this lane's noise stream at the row being worked
    if constexpr (NOISE) {
        uint64_t A, C;                                   // wave-uniform: the jump to the wave's first row
        noise::jump((uint32_t) __builtin_amdgcn_readfirstlane((int) (n_wave >> 6)), noise::kMul, noise::kInc, &A, &C);
        nx = A * noise::lane_start(nseed, nblock0 + (uint64_t) (block0 + blk), (uint32_t) lane) + C;
    }

    // ---- window builder: lane (c, g) prepares windows g, g+G, g+2G, ... of channel c ----
    constexpr int kPad = NCH <= 4 ? 4 : NCH <= 8 ? 8 : 16;   // lanes per window group
    constexpr int kGroups = 64 / kPad;
    constexpr int kRun = ROWS * H / kGroups;
    static_assert((ROWS * H) % kGroups == 0, "windows per chunk must split over the lane groups");
    const int c_raw = lane % kPad, wg = lane / kPad;
    const int wc = c_raw < NCH ? c_raw : 0;                  // surplus lanes shadow channel 0
    const bool w_store = c_raw < NCH;
    uint32_t w_k, w_nrev, w_nrot, w_dint;
    int32_t w_e1;
    uint64_t w_fr, w_dfr;
    {
        const gpsiq_qchan_t &q = qs[wc];
        const uint32_t n_row = n_wave + (uint32_t) wg * (uint32_t) kSpan;
        const unsigned __int128 T = (unsigned __int128) q.code_frac +
                                    (unsigned __int128) q.code_step * (unsigned __int128) n_row;
        const uint32_t A = (uint32_t) q.chip0 + (uint32_t) (uint64_t) (T >> GPSIQ_CODE_FRAC_BITS);
        w_fr = (uint64_t) T & kCodeFracMask;
        w_k = A % GPSIQ_CA_SEQ_LEN;                              // chip inside the period
        const uint32_t ic = q.icode + A / GPSIQ_CA_SEQ_LEN;
        // chips until the current nav bit ends, minus one (0..20459)
        w_e1 = (int32_t) ((20u - ic % 20u) * GPSIQ_CA_SEQ_LEN - w_k) - 1;
        // nav bits of this block, current bit in bit 31, the following ones below it
        w_nrev = __builtin_bitreverse32(q.nav_bits >> ((ic / 20u) & 31u));
        w_nrot = 0u - A;                                         // minus the rotation: only (-A) mod 32 matters
        // chips per builder step: kSpan*kGroups samples (<= 1024 samples at <= 0.5 chip, or
        // <= 512 samples at <= 1 chip: one period wrap at most)
        const unsigned __int128 step = (unsigned __int128) q.code_step * (unsigned) (kSpan * kGroups);
        w_dint = (uint32_t) (uint64_t) (step >> GPSIQ_CODE_FRAC_BITS);
        w_dfr = (uint64_t) step & kCodeFracMask;
    }

    // ---- per-lane NCO state of every channel (steps in SGPRs via scalar loads) -----
    const uint32_t n0 = n_wave + (uint32_t) lane;
    uint64_t P[NCH], Q[NCH], dP[NCH], dQ[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const bool have = c < nchan;
        const uint64_t p0 = have ? q_blk[c].carr_phase : 0u, ps = have ? (uint64_t) q_blk[c].carr_step : 0u;
        const uint64_t f0 = have ? q_blk[c].code_frac : 0u, cs = have ? q_blk[c].code_step : 0u;
        const uint64_t c0 = have ? (uint64_t) q_blk[c].chip0 : 0u;
        // BOTH keeps the 59-bit phase left-aligned in the word (it then wraps by itself, index in the top nine bits)
        constexpr int kAlign = BOTH ? 64 - GPSIQ_CARR_FRAC_BITS : 0;
        P[c] = (p0 + ps * (uint64_t) n0) << kAlign;
        Q[c] = (c0 << GPSIQ_CODE_FRAC_BITS) + f0 + cs * (uint64_t) n0;
        dP[c] = (ps * 64u) << kAlign;
        dQ[c] = cs * 64u;
    }

    const unsigned char *lut_b = reinterpret_cast<const unsigned char *>(&lut[0][0]);
    const uint32_t *w_row = &win[wave][H == 2 ? lane >> 5 : 0][0];   // upper half wave: second window of the row
    uint32_t *w_dst = &win[wave][wg][wc];

    // the clamp's lower bound, once per wave in a vector register of its own (as the result of an asm statement it is kept, not
    // formed again from the scalar register in every row).  The packed core has no register to spare for it (128 VGPRs: it would
    // spill) and forms it per row.
    [[maybe_unused]] int32_t l_neg = 0;
    if constexpr (LEVEL && FAST) asm("v_mov_b32 %0, %1" : "=v"(l_neg) : "s"(-(int32_t) lqmax));

    constexpr uint32_t kElem = FMT == GPSIQ_SC16 ? 4u : 2u;     // bytes of one stored sample

    // this lane's noise at the row being worked (mod 2^32); steps its stream on to the next row
    auto noise_row = [&](uint32_t &zi, uint32_t &zq) {
        const uint32_t w = noise::xsh_rr(nx);
        nx = nx * noise::kMul + noise::kInc;
        zi = (uint32_t) noise::z(nz, w & 0xffffu);
        zq = (uint32_t) noise::z(nz, w >> 16);
    };
    // what the plain-add core's sum becomes before the level stage or the store: the noise as one more term, the bias off
    auto fast_word = [&](uint32_t sum, uint32_t zi, uint32_t zq) -> uint32_t {
        if constexpr (NOISE && !LEVEL) {
            if (FMT == GPSIQ_SC08)
                // a 17th term in the 12-bit fields: I's spill bits (16..19) are cleared first, so its carry stays out of Q
                sum = (sum & ~0xf0000u) + ((zi & 0xfffu) << 4) + (zq << 20);
            else
                sum += zi + (zq << 16);                           // |I + zI| <= 32767 (the host's choice of core): no borrow into Q
        }
        return LFMT == GPSIQ_SC16 ? sum ^ 0x8000u : sum;          // take the bias off again: (I & 0xffff) | Q << 16
    };
    // the level stage (LEVEL kernels) and the store of one sample at o; iq = (I & 0xffff) | Q << 16 as the int16 store keeps it
    auto emit = [&](uint32_t iq, [[maybe_unused]] uint32_t zi, [[maybe_unused]] uint32_t zq, uint8_t *o, bool ok) {
        if constexpr (LEVEL) {
            // iq holds the noiseless sums as the int16 store would keep them.  Each comes out of the word sign-extended, the
            // noise is added in 32 bits (nothing wraps), then scale, round, clamp: the product needs more than 32 bits
            // (|A| < 2^19, mult < 2^24: v_mad_i64_i32), the quotient does not
            const int32_t ai = (int32_t) (int16_t) iq + (int32_t) zi, aq = ((int32_t) iq >> 16) + (int32_t) zq;
            const int32_t yi = (int32_t) (((int64_t) ai * (int64_t) (int32_t) lmult + 32768) >> 16);
            const int32_t yq = (int32_t) (((int64_t) aq * (int64_t) (int32_t) lmult + 32768) >> 16);
            // the clamp is one v_med3_i32 per component (written out: the compiler cannot know that -qmax <= qmax and emits
            // min, compare and select; a VOP3 instruction reads one scalar register at most, so -qmax sits in a vector register)
            uint32_t oi, oq;
            if constexpr (!FAST) l_neg = -(int32_t) lqmax;
            asm("v_med3_i32 %0, %1, %2, %3" : "=v"(oi) : "v"(yi), "v"(l_neg), "s"((int32_t) lqmax));
            asm("v_med3_i32 %0, %1, %2, %3" : "=v"(oq) : "v"(yq), "v"(l_neg), "s"((int32_t) lqmax));
            if (ok) {
                if (FMT == GPSIQ_SC16) *reinterpret_cast<uint32_t *>(o) = (oi & 0xffffu) | (oq << 16);
                else *reinterpret_cast<uint16_t *>(o) = (uint16_t) ((oi & 0xffu) | (oq << 8));
            }
        } else if (ok) {
            if (FMT == GPSIQ_SC16)
                *reinterpret_cast<uint32_t *>(o) = iq;                                        // gps.c:2842
            else                                                                             // bytes 1 and 3, see the LUT build
                *reinterpret_cast<uint16_t *>(o) = (uint16_t) __builtin_amdgcn_perm(iq, iq, 0x0c0c0301u);
        }
    };

    // ---- kTrip rows per loop trip (the plain-add cores) ----
    // One trip works rows r .. r + kTrip - 1 of a chunk off one window pointer and one store pointer: the rows' window reads and
    // stores differ in their immediate offsets only.  Within a row the LDS traffic runs under arithmetic that does not wait for
    // it: the gathers go out behind the address arithmetic, the NCO adds (which depend on nothing in flight) follow, and only
    // then does the sum wait for the gathers, in their order.  A row's window words are dead once the sixteen shifts have read
    // them, so the NEXT row's windows are read into them meanwhile (wv is carried from row to row and from trip to trip): half
    // way down the NCO adds, which measured 0.2-0.3 % faster than right behind the shifts (twenty LDS instructions in one burst).
    // A wave then covers its own LDS latency instead of leaving it to the other three of its SIMD.  The packed core has no
    // registers for a second set of window words (128 VGPRs) and keeps one row per trip; the 16-channel noise and level
    // kernels have none either (the noise stream and the level's operands take them: they would spill) and do the same.
    constexpr int kTrip = FAST && !(NOISE && NCH > 12) ? 4 : 1;
    static_assert(ROWS % kTrip == 0, "whole trips in a full chunk");
    static_assert(NCH % 4 == 0, "window words are read four at a time");
    typedef uint32_t win4 __attribute__((ext_vector_type(4)));
    auto read_windows = [&](const uint32_t *w, uint32_t (&wv)[NCH]) {
        const win4 *w4 = reinterpret_cast<const win4 *>(__builtin_assume_aligned(w, 16));
#pragma unroll
        for (int c = 0; c < NCH; c += 4) {
            const win4 v = w4[c / 4];
            wv[c] = v.x; wv[c + 1] = v.y; wv[c + 2] = v.z; wv[c + 3] = v.w;
        }
    };
    // w_at: window of the trip's first row (on return: of the row that wv holds, w_step words on);  o: the first row's sample
    [[maybe_unused]] auto trip_body = [&](const uint32_t *&w_at, uint32_t (&wv)[NCH], uint8_t *o, int w_step) {
#pragma unroll
        for (int j = 0; j < kTrip; ++j) {
            uint32_t t[NCH], g[NCH];
            [[maybe_unused]] uint32_t zi = 0, zq = 0;
#pragma unroll
            for (int c = 0; c < NCH; ++c) t[c] = wv[c] >> ((uint32_t) (Q[c] >> 56) & 31u);   // bit 0 = chip ^ nav bit of this lane
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if (BOTH) {
                    const uint32_t x = __builtin_amdgcn_alignbit(t[c], (uint32_t) (P[c] >> 32), 21u);
                    g[c] = *reinterpret_cast<const uint32_t *>(lut_b + c * 4096 + (x & 0xffcu));
                } else {
                    const uint32_t x = (t[c] << 26) + (uint32_t) (P[c] >> 32);
                    g[c] = *reinterpret_cast<const uint32_t *>(lut_b + c * 2048 + ((x >> 16) & 0x7fcu));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NOISE) noise_row(zi, zq);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if (c == NCH / 2) {
                    // the next row's windows, half way down the adds.  The last row of the trip reads ahead for the next trip;
                    // the last trip of a chunk has w_step == 0 and reads its own first row again, never past the chunk's windows
                    __builtin_amdgcn_sched_barrier(0);
                    if (j + 1 == kTrip) w_at += w_step;
                    read_windows(j + 1 == kTrip ? w_at : w_at + (j + 1) * (H * NCH), wv);
                    __builtin_amdgcn_sched_barrier(0);
                }
                P[c] += dP[c];
                Q[c] += dQ[c];
                // one add per row and word, in place: left to itself the compiler rewrites the trip's four adds of a word so
                // that several values of it are live at once, and the 16-channel kernels spill some 150 registers
                asm("" : "+v"(P[c]), "+v"(Q[c]));
            }
            __builtin_amdgcn_sched_barrier(0);
            uint32_t sum = 0u;
#pragma unroll
            for (int c = 0; c < NCH; ++c) sum += g[c];
            emit(fast_word(sum, zi, zq), zi, zq, o + (uint32_t) j * (64u * kElem), true);
        }
    };

    auto row_body = [&](int r, uint32_t n_chunk, bool check) {
        uint32_t iq;                                             // (I & 0xffff) | Q << 16, what the int16 store keeps
        [[maybe_unused]] uint32_t zi = 0, zq = 0;                // noise of this lane's sample, mod 2^32
        if constexpr (NOISE) noise_row(zi, zq);
        if (FAST) {
            uint32_t sum = 0u;                                    // int16: slot 0's entries carry a +0x8000 bias
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint32_t w = w_row[r * (H * NCH) + c];
                const uint32_t t = w >> ((uint32_t) (Q[c] >> 56) & 31u);        // bit 0 = chip ^ nav bit of this lane
                if (BOTH) {
                    // {strays, sign, index, 2 fraction bits}: sign and index make the word address in the 4 KB table
                    const uint32_t x = __builtin_amdgcn_alignbit(t, (uint32_t) (P[c] >> 32), 21u);
                    sum += *reinterpret_cast<const uint32_t *>(lut_b + c * 4096 + (x & 0xffcu));
                } else {
                    const uint32_t x = (t << 26) + (uint32_t) (P[c] >> 32);      // + half a cycle when that bit is set
                    const uint32_t a = (x >> 16) & 0x7fcu;
                    sum += *reinterpret_cast<const uint32_t *>(lut_b + c * 2048 + a);
                }
                P[c] += dP[c];
                Q[c] += dQ[c];
            }
            iq = fast_word(sum, zi, zq);
        } else {
            s16x2 acc0 = (s16x2) (0), acc1 = (s16x2) (0);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint32_t w = w_row[r * (H * NCH) + c];
                const uint32_t b = (uint32_t) (Q[c] >> 56);
                const uint32_t m = (uint32_t) __builtin_amdgcn_sbfe((int) w, b, 1u);
                const uint32_t sgn = m | 0x00010001u;
                const uint32_t a = (uint32_t) (P[c] >> 48) & 0x7fcu;
                const uint32_t v = *reinterpret_cast<const uint32_t *>(lut_b + c * 2048 + a);
                if (c & 1) acc1 = __builtin_bit_cast(s16x2, v) * __builtin_bit_cast(s16x2, sgn) + acc1;
                else       acc0 = __builtin_bit_cast(s16x2, v) * __builtin_bit_cast(s16x2, sgn) + acc0;
                P[c] += dP[c];
                Q[c] += dQ[c];
            }
            if constexpr (NOISE && !LEVEL) {
                constexpr int kPre = FMT == GPSIQ_SC08 ? 4 : 0;  // the int8 entries are pre-shifted by 4, see the LUT build
                acc0 = __builtin_bit_cast(s16x2, ((zi << kPre) & 0xffffu) | (zq << (16 + kPre))) + acc0;
            }
            iq = __builtin_bit_cast(uint32_t, acc0 + acc1);
        }
        const uint32_t n = n_chunk + (uint32_t) lane + (uint32_t) r * 64u;
        emit(iq, zi, zq, blk_dst + n * kElem, !check || n < (uint32_t) nsamp);
    };

    for (int row0 = 0; row0 < wave_rows; row0 += ROWS) {
        const uint32_t n_chunk = n_wave + (uint32_t) row0 * 64u;
        // windows of this chunk (the builder state carries over from the previous chunk).
        // A nav-bit edge comes by once in 20 ms (about 800 rows) per channel: a group of four windows
        // during which no lane of the wave gets near one needs no attention to the edge counter and the
        // nav word (with 16 channels about two groups in three).
        constexpr int kGrp = 4;
        static_assert(kRun % kGrp == 0, "window groups");
        const uint32_t reach = (uint32_t) kGrp * (w_dint + 1u) + 32u;      // chips a lane can advance in a group + one window
#pragma unroll 1
        for (int i0 = 0; i0 < kRun; i0 += kGrp) {
            if (__builtin_amdgcn_ballot_w64((uint32_t) w_e1 <= reach) == 0) {
                const uint32_t nrot0 = w_nrot;
                const uint32_t d0 = (uint32_t) ((int32_t) w_nrev >> 31);
#pragma unroll
                for (int i = i0; i < i0 + kGrp; ++i) {
                    const uint32_t lo = ext[wc][w_k >> 5], hi = ext[wc][(w_k >> 5) + 1];
                    const uint32_t S = __builtin_amdgcn_alignbit(hi, lo, w_k) ^ d0;   // 32 chips from chip k (shift uses k & 31)
                    // rotate left by A mod 32 (alignbit rotates right by its low 5 bits); an unused slot
                    // needs no masking: its LUT entries are all zero
                    if (w_store) w_dst[i * (kGroups * NCH)] = __builtin_amdgcn_alignbit(S, S, w_nrot);
                    w_fr += w_dfr;
                    const uint32_t adv = w_dint + (uint32_t) (w_fr >> GPSIQ_CODE_FRAC_BITS);
                    w_fr &= kCodeFracMask;
                    w_nrot -= adv;
                    const uint32_t k2 = w_k + adv;                        // adv < 1023: one period wrap at most
                    w_k = k2 - GPSIQ_CA_SEQ_LEN < k2 ? k2 - GPSIQ_CA_SEQ_LEN : k2;
                }
                w_e1 -= (int32_t) (nrot0 - w_nrot);                       // chips advanced in this group
            } else {
#pragma unroll
                for (int i = i0; i < i0 + kGrp; ++i) {
                    const uint32_t lo = ext[wc][w_k >> 5], hi = ext[wc][(w_k >> 5) + 1];
                    uint32_t S = __builtin_amdgcn_alignbit(hi, lo, w_k);
                    S ^= (uint32_t) ((int32_t) w_nrev >> 31);
                    // the window holds the start of the next nav bit when fewer than 32 chips of the
                    // current one are left
                    const bool edge = (uint32_t) w_e1 < 31u;
                    if (__builtin_expect(__builtin_amdgcn_ballot_w64(edge) != 0, 0)) {
                        if (edge && ((w_nrev ^ (w_nrev << 1)) >> 31)) S ^= 0xfffffffeu << w_e1;
                    }
                    if (w_store) w_dst[i * (kGroups * NCH)] = __builtin_amdgcn_alignbit(S, S, w_nrot);
                    w_fr += w_dfr;
                    const uint32_t adv = w_dint + (uint32_t) (w_fr >> GPSIQ_CODE_FRAC_BITS);
                    w_fr &= kCodeFracMask;
                    w_nrot -= adv;
                    const uint32_t k2 = w_k + adv;
                    w_k = k2 - GPSIQ_CA_SEQ_LEN < k2 ? k2 - GPSIQ_CA_SEQ_LEN : k2;
                    const int32_t e = w_e1 - (int32_t) adv;               // adv < 20460: one bit edge at most
                    const int32_t m = e >> 31;
                    w_e1 = e + (m & (int32_t) (20 * GPSIQ_CA_SEQ_LEN));
                    w_nrev <<= (uint32_t) m & 1u;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        int rows = wave_rows - row0;                         // the wave's last chunk may be partial
        rows = rows < ROWS ? rows : ROWS;
        if (n_chunk + (uint32_t) rows * 64u <= (uint32_t) nsamp) {
            const int rows_s = __builtin_amdgcn_readfirstlane(rows);       // the trip count is wave-uniform: keep it scalar
            int r = 0;
            if constexpr (kTrip > 1) {
                const int trips = rows_s / kTrip;
                if (trips > 0) {
                    const uint32_t *w_at = w_row;
                    uint32_t wv[NCH];
                    read_windows(w_at, wv);
                    uint32_t o_off = (n_chunk + (uint32_t) lane) * kElem;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
                    for (int t = trips; t > 0; --t) {
                        trip_body(w_at, wv, blk_dst + o_off, t > 1 ? kTrip * (H * NCH) : 0);
                        o_off += (uint32_t) kTrip * 64u * kElem;
                    }
                    r = trips * kTrip;
                }
            }
            // a partial chunk's last rows, one per trip
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (; r < rows_s; ++r) row_body(r, n_chunk, false);
        } else {                                             // the block ends inside this chunk
            const int in_block = (int) (((uint32_t) nsamp - n_chunk + 63u) >> 6);
            rows = rows < in_block ? rows : in_block;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int r = 0; r < rows; ++r) row_body(r, n_chunk, true);
        }
        // the next chunk overwrites this wave's windows: all lanes must be done reading
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
