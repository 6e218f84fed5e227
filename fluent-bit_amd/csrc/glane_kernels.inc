// glane_kernels.inc -- filter_grep in ONE pass: decide and copy (included by kernels_glane.hip inside namespace flbgpu, behind
// kdev.inc and lookback.inc).
//
// What it replaces: cb_grep_filter's loop (plugins/filter_grep/grep.c:286-392) -- decode the event, flb_ra_regex_match every rule
// (grep_filter_data :167-194, grep_filter_data_and_or :250-284), keep or drop the record -- which k_grep_match + k_scan + k_gather
// do in three launches that read the chunk once and the kept records a second time.  Here a wave stages its records in LDS (straight
// from HBM, no registers), a lane decides ITS record, the kept lengths are summed over the wave and the workgroup, the workgroup's
// place in the output comes from the look-back over the workgroups in front (lookback.inc), and the kept records leave LDS eight
// lanes a record: the chunk is read once, the kept records are written once.
//
// The lane's walk is written for what log events look like -- `92 92 d7 00 <sec> <nsec> 80` in front of a fixmap / map16 body whose
// keys are fixstr / str8 and whose values are strings, numbers, booleans or small containers of those -- on LDS pointers (the walkers
// of kdev.inc take generic pointers: every byte of a record in LDS was a flat load through the aperture), and the match-only
// automata step on bytes that come in four at a time with their four class lookups in flight together.  A record of any other shape
// (legacy events, metadata, bin / ext values, keys that are not strings, a timestamp the decoder hides, a record longer than the
// wave's LDS) is decided by the SAME functions k_grep_match runs (decode_event, grep_decide: kdev.inc), in this kernel, so that every
// record has one answer: the reference's.

#ifndef GL_WAVES_
#define GL_WAVES_ 4
#endif
constexpr int GL_TEXT_MAX = 15872;                // record bytes of a wave at most; a launch takes what 64 of ITS records need (GrepLaneArgs::text_cap),
                                                  // so that a chunk of short records leaves the LDS to more workgroups
constexpr int GL_WAVES = GL_WAVES_;               // waves of a workgroup: one look-back word and one copy of the rules' tables for them

constexpr int GL_PAR = 6;                         // automata stepped side by side
// what rule i's key resolves to, given the value object of its top-level name at v (GL_NONE: the name is not there): 1 a string
// (body, len), -1 nothing a pattern can match (flb_ra_regex_match answers -1), -2: not decidable here
DEV int gl_value(const GrepArgs &g, int i, LDS_AS const uint8_t *t, uint32_t v, uint32_t end, uint32_t &body, uint32_t &len) {
    const GrepRule &ru = g.rules[i];
    if (v == GL_NONE) return -1;
    if (ru.key.nsub > 0) {
        // `$k['a']['b']`: maps of string keys, the LAST entry of a name (src/flb_ra_key.c:151-236 as kdev.inc ra_descend restates it)
        const uint32_t b0 = t[v];
        const bool cont = (b0 >= 0x80 && b0 <= 0x9f) || b0 == 0xde || b0 == 0xdf || b0 == 0xdc || b0 == 0xdd;
        if (cont) {
            uint32_t cur = v;
            for (int s = 0; s < ru.key.nsub; s++) {
                if (ru.key.sub_is_index[s]) return -2;
                const uint32_t b = t[cur];
                uint32_t n, p;
                if (b >= 0x80 && b <= 0x8f) { n = b & 15; p = cur + 1; }
                else if (b == 0xde) { n = ((uint32_t) t[cur + 1] << 8) | t[cur + 2]; p = cur + 3; }
                else if (b >= 0x90 && b <= 0x9f) return -1;             // an array where a name is asked for: the lookup ends, nothing matched at this level
                else return -2;
                uint32_t found = GL_NONE;
                for (uint32_t e = 0; e < n; e++) {
                    uint32_t kb, kl;
                    const bool ks = gl_str(t, p, end, kb, kl);
                    const uint32_t kend = ks ? kb + kl : gl_skip(t, p, end);
                    if (kend == GL_NONE) return -2;
                    const uint32_t vend = gl_skip(t, kend, end);
                    if (vend == GL_NONE) return -2;
                    if (ks && kl > 32) return -2;
                    if (ks && kl == (uint32_t) ru.key.sub_len[s] && gl_key_eq(t, kb, ru.key.sub_str + ru.key.sub_off[s], kl)) found = kend;
                    p = vend;
                }
                if (found == GL_NONE) return -1;                        // ("try next entry" there: the levels can no longer all match, the lookup has no value)
                cur = found;
            }
            v = cur;
        }
    }
    if (!gl_str(t, v, end, body, len)) {
        // not a string: no match -- when it is one of the plain types; anything else the generic code names
        const uint32_t b = t[v];
        const bool plain = b <= 0x9f || b >= 0xe0 || b == 0xc0 || b == 0xc2 || b == 0xc3 || (b >= 0xca && b <= 0xd3) || b == 0xde || b == 0xdc;
        return plain ? -1 : -2;
    }
    return 1;
}

// The rules' tables in LDS are not upload_dfa's blobs as they stand: a row of the transition table gets one more column, the answer at
// the end of the text in that state (d_final), and a cell holds the NEXT ROW'S OFFSET (state x row width) -- a step is one addition and
// one read, the end of the text one more read, no multiplication.  0xFFFF (match whatever follows) and 0xFFFE (hand the value on) stay.

// the lane's record [rs, re) of the wave's LDS, walked once: hit[s] = the value object of slot s's name (its LAST entry), GL_NONE without one.
// 1 walked, -1 a record the decoder hides (an empty row), -2: not a plain log event (the caller runs decode_event / grep_decide on it)
DEV int gl_walk(const GrepLaneArgs &a, LDS_AS const uint8_t *t, uint32_t rs, uint32_t re, uint32_t (&hit)[GREP_SLOTS]) {
    if (rs == re) return -1;                                            // a row an earlier filter emptied
    if (re - rs < 14 || *(LDS_AS gl_u32u *) (t + rs) != 0x00d79292u || t[rs + 12] != 0x80) return -2;
    const uint32_t sec = __builtin_bswap32(*(LDS_AS gl_u32u *) (t + rs + 4)), nsec = __builtin_bswap32(*(LDS_AS gl_u32u *) (t + rs + 8));
    if (sec >= 0xfffffffeu || nsec >= 1000000000u) return -2;
    uint32_t p = rs + 13, n;
    const uint32_t b = t[p];
    if (b >= 0x80 && b <= 0x8f) { n = b & 15; p += 1; }
    else if (b == 0xde && p + 3 <= re) { n = ((uint32_t) t[p + 1] << 8) | t[p + 2]; p += 3; }
    else return -2;
    // every rule key with one walk: the value of its LAST entry
    #pragma unroll
    for (int s = 0; s < GREP_SLOTS; s++) hit[s] = GL_NONE;
    const int ns = a.nslots;
    for (uint32_t e = 0; e < n; e++) {
        uint32_t kb, kl;
        if (!gl_str(t, p, re, kb, kl)) return -2;                       // (a key that is no string: legal, rare, the generic walk's)
        const uint32_t v = kb + kl;
        const uint32_t vend = gl_skip(t, v, re);
        if (vend == GL_NONE) return -2;
        if (kl >= 1 && kl <= 32) {
            // the name's first eight bytes once (what stands behind the name is masked off), every slot compares registers; longer names go on
            const uint32_t k0 = *(LDS_AS gl_u32u *) (t + kb), k1 = *(LDS_AS gl_u32u *) (t + kb + 4);
            const uint32_t m0 = kl >= 4 ? 0xFFFFFFFFu : (1u << (8 * kl)) - 1, m1 = kl >= 8 ? 0xFFFFFFFFu : kl <= 4 ? 0u : (1u << (8 * (kl - 4))) - 1;
            #pragma unroll
            for (int s = 0; s < GREP_SLOTS; s++) {
                if (s < ns && kl == (uint32_t) a.slot_klen[s] && (k0 & m0) == a.slot_kw[s][0] && (k1 & m1) == a.slot_kw[s][1]) {
                    // (a name of more than eight bytes: its other dwords, each index a constant -- the argument block is read with scalar loads)
                    uint32_t diff = 0;
                    if (kl > 8) {
                        #pragma unroll
                        for (int j = 2; j < 8; j++) {
                            const uint32_t left = kl > 4u * j ? kl - 4u * j : 0u, m = left >= 4 ? 0xFFFFFFFFu : left ? (1u << (8 * left)) - 1 : 0u;
                            diff |= (*(LDS_AS gl_u32u *) (t + kb + 4 * j) & m) ^ a.slot_kw[s][j];
                        }
                    }
                    if (diff == 0) hit[s] = v;                           // (the last entry of a name wins: flb_ra_key.c's backward lookup)
                }
            }
        }
        p = vend;
    }
    if (p != re) return -2;                                             // (the generic decode says what is wrong with it)
    return 1;
}

// one filter's rules on the walked record: 1 keep, 0 drop, -2: not decidable here
DEV int gl_rules(const GrepLaneArgs &a, const GrepArgs &g, LDS_AS const uint8_t *t, uint32_t re, const uint32_t (&hit)[GREP_SLOTS], LDS_AS const uint8_t *tabs, unsigned long long *ph) {
    unsigned long long t0_ = a.prof ? __builtin_readcyclecounter() : 0;
    // the rules' automata, GL_PAR of them side by side (their LDS reads in flight together: the walk of one value is a chain of dependent
    // reads, the values of different rules are independent), then the verdict in the rules' order (grep.c:167-194 legacy, :250-284 AND / OR)
    unsigned long long matched = 0;                                     // bit i: rule i's pattern matches its value
    for (int g0 = 0; g0 < g.nrules; g0 += GL_PAR) {
        uint32_t pos[GL_PAR], len[GL_PAR], st[GL_PAR], width[GL_PAR], res[GL_PAR];
        LDS_AS const uint8_t *blob[GL_PAR];
        uint32_t maxlen = 0;
        #pragma unroll
        for (int j = 0; j < GL_PAR; j++) {
            pos[j] = 0; len[j] = 0; st[j] = 0; width[j] = 0; res[j] = RX_NOMATCH; blob[j] = tabs;
            const int i = g0 + j;
            if (i < g.nrules) {
                const uint32_t slot = g.rule_slot[i];
                uint32_t v = hit[0];
                #pragma unroll
                for (int s = 1; s < GREP_SLOTS; s++) if (slot == (uint32_t) s) v = hit[s];
                uint32_t body = 0, l = 0;
                const int vr = gl_value(g, i, t, v, re, body, l);
                if (vr == -2) return -2;
                const GrepRule &ru = g.rules[i];
                width[j] = (uint32_t) ru.dfa.ncls + 1;
                blob[j] = tabs + g.rule_lds_off[i];
                st[j] = (uint32_t) ru.dfa.d_init * width[j];
                if (vr == 1) { pos[j] = body; len[j] = l; res[j] = 0xFFu; if (l > maxlen) maxlen = l; }      // 0xFF: the automaton is running
            }
        }
        if (a.prof) { const unsigned long long n_ = __builtin_readcyclecounter(); ph[2] += n_ - t0_; t0_ = n_; }
        for (uint32_t k = 0; k < maxlen; k += 4) {
            #pragma unroll
            for (int j = 0; j < GL_PAR; j++) {
                if (res[j] == 0xFFu && k < len[j]) {
                    LDS_AS const uint16_t *dd = (LDS_AS const uint16_t *) (blob[j] + 256);
                    const uint32_t w = *(LDS_AS gl_u32u *) (t + pos[j] + k), left = len[j] - k;
                    const uint32_t c0 = blob[j][w & 255], c1 = blob[j][(w >> 8) & 255], c2 = blob[j][(w >> 16) & 255], c3 = blob[j][w >> 24];
                    uint32_t n = dd[st[j] + c0], s_ = n;
                    if (n < 0xFFFE && left > 1) { n = dd[s_ + c1]; if (n < 0xFFFE) s_ = n; }
                    if (n < 0xFFFE && left > 2) { n = dd[s_ + c2]; if (n < 0xFFFE) s_ = n; }
                    if (n < 0xFFFE && left > 3) { n = dd[s_ + c3]; if (n < 0xFFFE) s_ = n; }
                    if (n >= 0xFFFE) res[j] = n == 0xFFFF ? (uint32_t) RX_MATCH : (uint32_t) RX_POISON;
                    else st[j] = s_;
                }
            }
        }
        if (a.prof) { const unsigned long long n_ = __builtin_readcyclecounter(); ph[3] += n_ - t0_; t0_ = n_; }
        #pragma unroll
        for (int j = 0; j < GL_PAR; j++) {
            const int i = g0 + j;
            if (i < g.nrules) {
                uint32_t m = res[j];
                if (m == 0xFFu) m = ((LDS_AS const uint16_t *) (blob[j] + 256))[st[j] + width[j] - 1];       // the end of the text in this state
                if (m == (uint32_t) RX_POISON) m = rx_match_handed_on(g.rules[i].utf8, (const uint8_t *) (t + pos[j]), len[j]) ? RX_MATCH : RX_NOMATCH;
                if (m == (uint32_t) RX_MATCH) matched |= 1ull << i;
            }
        }
    }
    bool keep = true;
    const int op = g.logical_op;
    if (op == OP_LEGACY) {
        for (int i = 0; i < g.nrules; i++) {
            const int type = g.rules[i].type;
            if (!((matched >> i) & 1)) { if (type == GREP_REGEX) { keep = false; break; } }
            else { keep = (type != GREP_EXCLUDE); break; }
        }
    }
    else if (g.nrules > 0) {
        // (the reference's loop ends at the first rule that matches (OR) / does not (AND): `found` is then "any" / "all", and the type
        // is one for all the rules -- grep.c:90-98)
        const unsigned long long all = g.nrules >= 64 ? ~0ull : ((1ull << g.nrules) - 1);
        const bool found = op == OP_OR ? matched != 0 : matched == all;
        keep = (g.rules[0].type == GREP_REGEX) ? found : !found;
    }
    return keep ? 1 : 0;
}

#ifndef GL_MINW_
#define GL_MINW_ 2
#endif
__global__ void __launch_bounds__(64 * GL_WAVES, GL_MINW_) k_grep_lane(GrepLaneArgs a) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t GL_TEXT = a.text_cap, GL_LDS = GL_TEXT + 64;          // (multiples of 16)
    LDS_AS uint8_t *text = (LDS_AS uint8_t *) g_lds + (size_t) wave * GL_LDS;
    LDS_AS uint32_t *wg_tot = (LDS_AS uint32_t *) ((LDS_AS uint8_t *) g_lds + GL_WAVES * GL_LDS);                           // [GL_WAVES]
    LDS_AS unsigned long long *wg_word = (LDS_AS unsigned long long *) ((LDS_AS uint8_t *) g_lds + GL_WAVES * GL_LDS + 32);  // ticket, base, stuck
    LDS_AS uint8_t *tabs = (LDS_AS uint8_t *) g_lds + GL_WAVES * GL_LDS + 64;
    const uint8_t *data_end = a.g.data + a.g.bytes;
    const uint32_t R = a.rows_per_tile;
    const uint64_t nunits = (a.ntiles + GL_WAVES - 1) / GL_WAVES;
    // the rules' tables, one copy for the workgroup, in the layout the lanes step on (above gl_rules); both filters' when two run as one
    for (int which = 0; which < (a.two ? 2 : 1); which++) {
        const GrepArgs &g = which ? a.g2 : a.g;
        for (int i = 0; i < g.nrules; i++) {
            const DevDfa &df = g.rules[i].dfa;
            LDS_AS uint8_t *dst = tabs + g.rule_lds_off[i];
            LDS_AS uint16_t *dd = (LDS_AS uint16_t *) (dst + 256);
            const uint32_t ncls = (uint32_t) df.ncls, nD = (uint32_t) df.nD, width = ncls + 1;
            for (uint32_t k = threadIdx.x; k < 256; k += blockDim.x) dst[k] = df.cls[k];
            for (uint32_t k = threadIdx.x; k < nD * width; k += blockDim.x) {
                const uint32_t row = k / width, col = k - row * width;
                uint32_t v;
                if (col == ncls) v = df.d_final[row];
                else { v = df.ddelta[row * ncls + col]; if (v < 0xFFFEu) v *= width; }
                dd[k] = (uint16_t) v;
            }
        }
    }
    uint32_t n_dec = 0, n_keep = 0, n_keep2 = 0;
    unsigned long long bytes1 = 0;                                      // (two filters: the bytes the first one keeps, for its statistics)
    unsigned long long stamp = 0, ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // (a.prof: cycles per phase -- 0 staging, 1 walk, 2 values, 3 automata, 4 the lane's whole decision, 5 look-back, 6 copy)
#define GL_STAMP(i) do { if (a.prof) { const unsigned long long now_ = __builtin_readcyclecounter(); ph[i] += now_ - stamp; stamp = now_; } } while (0)
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) wg_word[0] = atomicAdd(a.ticket, 1ull);
        __syncthreads();
        const uint64_t unit = wg_word[0];
        if (unit >= nunits) break;
        const uint64_t tile = unit * GL_WAVES + wave;
        const bool live = tile < a.ntiles;
        if (a.prof) stamp = __builtin_readcyclecounter();
        const uint64_t r0 = live ? tile * R : 0;
        const uint32_t nrows = live ? (uint32_t) ((a.g.n - r0) < R ? (a.g.n - r0) : R) : 0;
        uint64_t o0 = 0, o1 = 0;
        if (lane < nrows) { o0 = a.g.row_off[r0 + lane]; o1 = a.g.row_off[r0 + lane + 1]; }
        const uint64_t g0 = __shfl(o0, 0, 64);
        const uint32_t align = (uint32_t) ((uintptr_t) (a.g.data + g0) & 15);
        const uint64_t base = g0 - align;                               // (the host checks that the chunk itself is 16-byte aligned)
        const bool have = lane < nrows && (o1 - base) <= (uint64_t) GL_TEXT;
        const uint32_t nfit = (uint32_t) __popcll(__ballot(have));      // offsets rise: the records that fit are the first nfit
        const uint32_t rs = have ? (uint32_t) (o0 - base) : 0, re = have ? (uint32_t) (o1 - base) : 0;
        const uint32_t hi = jt_readlane(nfit ? (uint32_t) __shfl((int) re, (int) (nfit - 1), 64) : align, 0);
        // ---- the records into LDS, straight from HBM
        {
            const uint8_t *src = a.g.data + base;
            const uint32_t nchunk = (hi + 16 + 15) >> 4;
            if (src + (size_t) nchunk * 16 <= data_end) {
#if defined(__HIP_DEVICE_COMPILE__)
                for (uint32_t u0 = 0; u0 < nchunk; u0 += 64)
                    if (u0 + lane < nchunk)
                        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *) (src + (size_t) (u0 + lane) * 16),
                                                         (void __attribute__((address_space(3))) *) (text + (size_t) u0 * 16), 16, 0, 0);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            }
            else {
                for (uint32_t u = lane; u < nchunk; u += 64) {
                    const uint8_t *p = src + (size_t) u * 16;
                    v4u32 v;
                    if (p + 16 <= data_end) v = *(const v4u32 *) p;
                    else {
                        uint32_t t4[4] = {0, 0, 0, 0};
                        for (int q = 0; q < 16 && p + q < data_end; q++) t4[q >> 2] |= (uint32_t) p[q] << (8 * (q & 3));
                        v.x = t4[0]; v.y = t4[1]; v.z = t4[2]; v.w = t4[3];
                    }
                    *(LDS_AS v4u32 *) (text + (size_t) u * 16) = v;
                }
            }
        }
        JT_SYNC();
        GL_STAMP(0);
        // ---- a lane decides its record
        uint32_t flags = RF_VALID | RF_SKIP, keeplen = 0;
        if (lane < nrows) {
            const uint64_t r = r0 + lane;
            // d: 1 the first filter keeps it, 0 drops it, -1 hidden / bad; d2 likewise for the second filter of a pair (it sees what the first keeps)
            uint32_t hit[GREP_SLOTS];
            unsigned long long tw_ = a.prof ? __builtin_readcyclecounter() : 0;
            int d = have ? gl_walk(a, text, rs, re, hit) : -2, d2 = 1;
            if (a.prof) ph[1] += __builtin_readcyclecounter() - tw_;
            if (d == 1) {
                d = gl_rules(a, a.g, text, re, hit, tabs, ph);
                if (d == 1 && a.two) d2 = gl_rules(a, a.g2, text, re, hit, tabs, ph);
                if (d2 == -2) d = -2;
            }
            if (d == -2) {
                // any other shape, or a record longer than the wave's LDS: the functions k_grep_match runs
                const uint8_t *rec = have ? (const uint8_t *) (text + rs) : a.g.data + o0, *rec_end = rec + (o1 - o0);
                Event ev = decode_event(rec, rec_end, true);
                bool keep = false, keep2 = true;
                if (!(ev.flags & (RF_BAD | RF_SKIP))) {
                    bool valid = false;
                    keep = grep_decide(a.g, ev, &valid, (LDS_AS const uint8_t *) nullptr, r, rec);     // (tables from device memory: the LDS copy has the lanes' layout)
                    if (!valid) valid = mp_skip(ev.body, rec_end, 1) == rec_end;
                    if (!valid) ev.flags = RF_BAD;
                    else if (keep && a.two) { bool v2 = false; keep2 = grep_decide(a.g2, ev, &v2, (LDS_AS const uint8_t *) nullptr, r, rec); }
                }
                else if ((ev.flags & RF_SKIP) && rec != rec_end && mp_skip(ev.body, rec_end, 1) != rec_end) ev.flags = RF_BAD;
                flags = ev.flags;
                d = (ev.flags & (RF_BAD | RF_SKIP)) ? -1 : (keep ? 1 : 0);
                d2 = keep2 ? 1 : 0;
            }
            else if (d >= 0) flags = RF_VALID;
            if (flags & RF_BAD) atomicMin(a.g.first_bad, (unsigned long long) r);
            else if (d >= 0) {
                n_dec++;
                if (d == 1) { n_keep++; bytes1 += o1 - o0; if (d2 == 1) { n_keep2++; keeplen = (uint32_t) (o1 - o0); } }
            }
            a.g.status[r] = flags;
            a.g.keep_len[r] = keeplen;
        }
        GL_STAMP(4);
        // ---- the kept records' places
        const uint32_t rowincl = jt_dpp_add(keeplen);
        const uint32_t total = jt_readlane(rowincl, 63);
        if (lane == 0) wg_tot[wave] = total;
        __syncthreads();
        if (wave == 0) {
            unsigned long long mine = 0;
            for (int w = 0; w < GL_WAVES; w++) mine += wg_tot[w];
            bool stk = false;
            const uint64_t prefix = lb_unit_base(a.unit_state, unit, mine, lane, stk);
            if (lane == 0) { wg_word[1] = prefix; wg_word[2] = stk ? 1 : 0; }
        }
        __syncthreads();
        uint64_t gbase = wg_word[1];
        const bool stuck = wg_word[2] != 0;
        for (uint32_t w = 0; w < wave; w++) gbase += wg_tot[w];
        GL_STAMP(5);
        const bool room = !stuck && gbase + total <= a.out_cap;
        const uint32_t rowoff = rowincl - keeplen;
        if (lane < nrows) a.off_out[r0 + lane] = gbase + rowoff;
        if (lane == 0) {
            // (a.words = &counts[MW_LANE_BYTES]: words[0] is that slot, words[1] the one behind it, MW_LANE_FAIL)
            if (!room) atomicAdd(&a.words[1], stuck ? (1ull << 32) : 1ull);
            if (live && tile == a.ntiles - 1) { a.off_out[a.g.n] = gbase + total; a.words[0] = gbase + total; }
        }
        // ---- the kept records leave: eight lanes a record, 32 bytes a lane
        if (room && total) {
            typedef v4u32 v4un __attribute__((aligned(1)));
            uint8_t *out = a.out + gbase;
            const uint32_t oct = lane >> 3, ol = lane & 7;
            for (uint32_t j0 = 0; j0 < nrows; j0 += 8) {
                const int j = (int) (j0 + oct);
                const uint32_t bl = __shfl(keeplen, j, 64), so = __shfl(rs, j, 64), dof = __shfl(rowoff, j, 64);
                const uint64_t go = __shfl(o0, j, 64);
                const bool inl = __shfl((int) have, j, 64) != 0;
                if (j < (int) nrows && bl) {
                    uint8_t *dst = out + dof;
                    if (!inl) {
                        // a record that did not fit in LDS: from the chunk
                        const uint8_t *sp = a.g.data + go;
                        for (uint32_t o = ol * 16; o < bl; o += 128) {
                            if (o + 16 <= bl) *(v4un *) (dst + o) = *(const v4un *) (sp + o);
                            else for (uint32_t q = o; q < bl; q++) dst[q] = sp[q];
                        }
                    }
                    else if (bl < 32) { if (ol == 0) for (uint32_t q = 0; q < bl; q++) dst[q] = text[so + q]; }
                    else {
                        for (uint32_t o = ol * 32; o < bl; o += 256) {
                            const uint32_t at = o + 32 > bl ? bl - 32 : o;                 // the last step of a record overlaps the one in front
                            LDS_AS uint8_t *sp = text + so + at;
                            v4u32 w, x;
                            w.x = *(LDS_AS gl_u32u *) sp; w.y = *(LDS_AS gl_u32u *) (sp + 4); w.z = *(LDS_AS gl_u32u *) (sp + 8); w.w = *(LDS_AS gl_u32u *) (sp + 12);
                            x.x = *(LDS_AS gl_u32u *) (sp + 16); x.y = *(LDS_AS gl_u32u *) (sp + 20); x.z = *(LDS_AS gl_u32u *) (sp + 24); x.w = *(LDS_AS gl_u32u *) (sp + 28);
                            *(v4un *) (dst + at) = w; *(v4un *) (dst + at + 16) = x;
                        }
                    }
                }
            }
        }
        JT_SYNC();
        GL_STAMP(6);
    }
    if (a.prof && lane == 0) for (int i = 0; i < 8; i++) atomicAdd(&a.prof[i], ph[i]);
#undef GL_STAMP
    // one pair of atomics per wave
    for (int o = 32; o > 0; o >>= 1) {
        n_dec += __shfl_down(n_dec, o, 64); n_keep += __shfl_down(n_keep, o, 64); n_keep2 += __shfl_down(n_keep2, o, 64); bytes1 += __shfl_down(bytes1, o, 64);
    }
    if (lane == 0) {
        if (n_dec) atomicAdd(&a.g.counts[MW_DECODED], (unsigned long long) n_dec);
        if (n_keep) atomicAdd(&a.g.counts[MW_KEPT], (unsigned long long) n_keep);
        if (a.two) { if (n_keep2) atomicAdd(&a.g.counts[MW_KEPT2], (unsigned long long) n_keep2); if (bytes1) atomicAdd(&a.g.counts[MW_BYTES1], bytes1); }
    }
}

// the longest run of R rows (bytes, with the 15 a tile may stand off an aligned address): what a wave's LDS has to hold
__global__ void __launch_bounds__(256) k_tile_max(const uint64_t *row_off, uint64_t n, uint32_t R, unsigned long long *out) {
    const uint64_t tiles = (n + R - 1) / R;
    unsigned long long m = 0;
    for (uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; t < tiles; t += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t r1 = (t + 1) * R < n ? (t + 1) * R : n;
        const unsigned long long b = row_off[r1] - row_off[t * R] + 15;
        m = b > m ? b : m;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long x = __shfl_xor(m, o, 64); m = x > m ? x : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
void launch_tile_max(const uint64_t *row_off, uint64_t n, uint32_t R, unsigned long long *out, hipStream_t st) {
    uint64_t blocks = ((n + R - 1) / R + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_tile_max, dim3((unsigned) blocks), dim3(256), 0, st, row_off, n, R, out);
}

void launch_grep_lane(const GrepLaneArgs &a, int cus, hipStream_t st) {
    const size_t lds = (size_t) GL_WAVES * (a.text_cap + 64) + 64 + a.g.rules_lds_total + (a.two ? a.g2.rules_lds_total : 0);
    (void) hipFuncSetAttribute((const void *) k_grep_lane, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
    uint32_t per_cu = (uint32_t) (160 * 1024 / lds);
    if (per_cu > 4 * GL_MINW_ / GL_WAVES) per_cu = 4 * GL_MINW_ / GL_WAVES;      // (the kernel's registers: GL_MINW_ waves a SIMD)
    const uint64_t nunits = (a.ntiles + GL_WAVES - 1) / GL_WAVES;
    uint64_t grid = (uint64_t) cus * (per_cu ? per_cu : 1);
    if (grid > nunits) grid = nunits;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_grep_lane, dim3((unsigned) grid), dim3(64 * GL_WAVES), lds, st, a);
}
int grep_lane_text_max() { return GL_TEXT_MAX; }
uint64_t grep_lane_units(uint64_t ntiles) { return (ntiles + GL_WAVES - 1) / GL_WAVES; }
uint32_t grep_lane_table_bytes(uint32_t nD, uint32_t ncls) { return (256 + nD * (ncls + 1) * 2 + 15) & ~15u; }
uint32_t grep_lane_table_room() { return 24576; }
