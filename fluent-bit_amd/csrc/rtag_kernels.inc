// rtag_kernels.inc -- filter_rewrite_tag (plugins/filter_rewrite_tag/rewrite_tag.c:356-557, src/flb_record_accessor.c:456-699): a lane
// per record, three launches around the shared scan.
//   k_rtag_match    decodes the row, walks the rules in order, looks each rule's KEY up (ra_lds.inc: the last STR key of that name,
//                   then the sub-keys) and runs the rule's match automaton on a STR value; the first match wins.  Writes the rule per
//                   row, whether the row is emitted and the bytes it keeps in the output if the emitter takes it.
//   k_rtag<false>   emitted rows only: the capture walk where the rule's template reads a `$n` (spans into the columns of the
//                   EMITTED row, so the scratch and the columns are as many as the emissions, not as the chunk), then the tag's length.
//   k_rtag<true>    emitted rows only: the tag into the row's own room of the tag arena, and the row's entry of the emitted table.
// ONE function, rt_compose, writes a tag into whatever sink it is given: k_rtag<false> hands it a CountSink, k_rtag<true> an RtSink that
// never stores outside [tag_off[r], tag_off[r + 1]).  A row whose written length is not its sized length is counted, not written past.
// The kept records are copied by k_gather (kernels.hip), as filter_grep's are: emit_raw_record copies the record as it is.
// Included inside namespace flbgpu after kdev.inc, lane_rows.inc, ra_lds.inc and fmt_dev.inc.

struct RtTable {
    const LDS_AS uint32_t *w;       // the table's words in LDS
    int nrules;
};

// the emit pass's sink: [p, limit) is the row's room.  Nothing is stored at or past limit; p keeps counting.
struct RtSink {
    uint8_t *p, *limit;
    bool over = false;
    DEV RtSink(uint8_t *dst, uint8_t *lim) : p(dst), limit(lim) {}
    DEV void put(uint32_t b) {
        if (p < limit) *p = (uint8_t) b; else over = true;
        p++;
    }
    DEV void copy(const uint8_t *src, uint32_t len) {
        const uint64_t room = p < limit ? (uint64_t) (limit - p) : 0;
        const uint32_t n = room < len ? (uint32_t) room : len;
        ByteSink bs(p);
        bs.copy(src, n);
        if (n < len) over = true;
        p += len;
    }
    // the first nbytes (<= 16) of w, byte by byte: nothing behind the row's room is touched
    DEV void put16(const v4u32 w, uint32_t nbytes) { for (uint32_t i = 0; i < nbytes; i++) put(v4_byte(w, i)); }
};

// the match automaton of a rule on the bytes of a value (flb_regex_do is a search: a match anywhere)
DEV bool rt_match(const GrepRule &ru, const uint8_t *s, uint32_t len) {
    int m = dfa_match(ru.dfa.cls, ru.dfa.ddelta, ru.dfa.d_final, ru.dfa.ncls, ru.dfa.d_init, s, len);
    if (m == RX_POISON) m = rx_match_handed_on(ru.utf8, s, len) ? RX_MATCH : RX_NOMATCH;
    return m == RX_MATCH;
}

// flb_ra_regex_match (src/flb_record_accessor.c:753-764) of rule ri: the STR value its KEY names, nullptr when there is none
DEV const uint8_t *rt_key_value(const RtTable &tb, uint32_t ri, const uint8_t *body, const uint8_t *end, uint32_t &vlen) {
    const LDS_AS uint32_t *r = tb.w + RT_RULE_WORDS * ri;
    if (r[0] & RT_INERT) return nullptr;
    const uint8_t *v = ra_lds_path(tb.w, tb.w + (r[2] >> 2), r[1], tb.w + (r[3] >> 2), (r[0] >> 8) & 0xffu, body, end, true);
    if (!v) return nullptr;
    Tok t = mp_tok(v, end);
    if (t.type != T_STR) return nullptr;
    vlen = t.len;
    return t.next;
}

// the capture walk of a rule on its value (kdev.inc try_parser without the parser's fields): spans of groups 1 .. 9 through
// slot2cap, group 0 from the walk's own start and end.  false: no match, or scratch the host sized too small.
template <class CAP>
DEV bool rt_capture(const RtagCap &ps, const uint8_t *val, uint32_t vlen, uint16_t *chk, uint32_t chk_len, uint32_t nfa_off, CAP &caps) {
    if (vlen / CHK_STEP + 2 > chk_len) return false;
    bool use_utf8 = false;
    uint32_t wlen = vlen;
    const HotTabs<false> hot = hot_global(ps.ascii);
    int best = ps.ascii.stub ? -2 : rx_reverse(hot, ps.ascii.r_info, val, vlen, chk);
    if (best == -2 && ps.utf8.nfa_on) {
        if (nfa_off + nfa_chk_words(ps.utf8.nfa, vlen) * 2 > chk_len) return false;
        const uint32_t ln = threadIdx.x & 63;
        int start = -1;
        const int e = nfa_capture(ps.utf8.nfa, val, vlen, (uint32_t *) (chk - ln + (size_t) nfa_off * 64) + ln, ps.slot2cap, caps, &start);
        if (e < 0) return false;
        caps.set(0, (uint32_t) start);
        caps.set(1, (uint32_t) e);
        return true;
    }
    const HotTabs<false> hu = hot_global(ps.utf8);
    if (best == -2) {
        use_utf8 = true;
        wlen = u8_walk_len(val, vlen);
        best = ps.utf8.wide ? rx_reverse(hot_global_wide(ps.utf8), ps.utf8.r_info, val, wlen, chk, vlen)
                            : rx_reverse(hu, ps.utf8.r_info, val, wlen, chk, vlen);
    }
    if (best < 0) return false;
    const int endb = !use_utf8 ? rx_forward(ps.ascii, hot, val, vlen, best, chk, ps.slot2cap, caps)
                   : ps.utf8.wide ? rx_forward(ps.utf8, hot_global_wide(ps.utf8), val, wlen, best, chk, ps.slot2cap, caps, vlen)
                                  : rx_forward(ps.utf8, hu, val, wlen, best, chk, ps.slot2cap, caps, vlen);
    if (endb < 0) return false;
    caps.set(0, (uint32_t) best);
    caps.set(1, (uint32_t) endb);
    if (wlen != vlen) {
        // the boundary behind a truncated last character is the end of the real text
        for (uint32_t f = 0; f < RT_CAP_COLS; f++) if (caps.get(f) == wlen) caps.set(f, vlen);
    }
    return true;
}

template <class S> struct RtDst { S &s; DEV void put(uint32_t c) { s.put(c); } };
// snprintf(str, sizeof(str) - 1, ...) into char str[32] (src/flb_record_accessor.c:560-569): 30 characters at most reach the buffer
struct RtF30 {
    uint8_t c[30];
    uint32_t n = 0;
    DEV void put(uint32_t b) { if (n < 30) c[n] = (uint8_t) b; n++; }
};

// ra_translate_tag_part (src/flb_record_accessor.c:488-521): the id-th dot-separated part of the tag
template <class S> DEV void rt_tag_part(S &s, const uint8_t *tag, uint32_t tag_len, int32_t want) {
    uint32_t i = 0;
    int32_t id = -1;
    while (i < tag_len) {
        uint32_t e = 0;
        while (i + e < tag_len && ld8(tag + i + e) != '.') e++;
        if (i + e >= tag_len) {                    // no further dot
            if (i == 0) break;
            e = tag_len - i;
        }
        id++;
        if (want == id) { s.copy(tag + i, e); return; }
        i += e + 1;
    }
    if (want == 0 && id == -1 && i < tag_len) s.copy(tag, tag_len);      // no dots in the tag
}

// ra_translate_keymap (src/flb_record_accessor.c:531-619) of the value at v
template <class S> DEV void rt_value(S &s, const uint8_t *v, const uint8_t *end) {
    Tok t = mp_tok(v, end);
    switch (t.type) {
    case T_STR: s.copy(t.next, t.len); break;
    case T_BOOL: if (t.u) j_lit(s, "true", 4); else j_lit(s, "false", 5); break;
    case T_NIL: j_lit(s, "null", 4); break;
    case T_UINT: case T_NINT: { RtDst<S> o{s}; nc::fmt_ld((int64_t) t.u, o); break; }          // "%ld" of via.i64
    case T_F32: case T_F64: {
        const uint64_t bits = t.type == T_F64 ? t.u : (uint64_t) __double_as_longlong((double) __uint_as_float((uint32_t) t.u));
        // "%f" of 31 characters and more: 30 of them, then the terminator snprintf wrote behind them goes into the tag too
        // (flb_sds_cat_safe of len, or of sizeof(str) - 1, bytes: :563-568)
        RtF30 f;
        RtDst<RtF30> o{f};
        const int n = nc::fmt_f6(bits, o, 400);
        const uint32_t m = n < 30 ? (uint32_t) n : 30u;
        for (uint32_t i = 0; i < m; i++) s.put(f.c[i]);
        if (n >= 31) s.put(0);
        break;
    }
    case T_BIN:
        for (uint32_t i = 0; i < t.len; i++) {
            const uint32_t b = ld8(t.next + i), h = b >> 4, l = b & 15;
            s.put(h < 10 ? '0' + h : 'a' + h - 10); s.put(l < 10 ? '0' + l : 'a' + l - 10);
        }
        break;
    case T_MAP: {
        // flb_msgpack_to_json_str(1024, &o, escape_unicode = TRUE) (msgpack2json, src/flb_pack.c:993-1140): a key that occurs again
        // later in its map is left out with its value, the walker that looks ahead from every key
        JsonFmtCfg cfg;
        cfg.json_format = 0; cfg.date_format = 0; cfg.escape_unicode = 1; cfg.nan_to_null = 0; cfg.has_date = 0; cfg.date_key_is_internal = 0;
        cfg.date_key_len = 0; cfg.date_key = nullptr;
        const uint8_t *e = nullptr;
        (void) j_walk<DUP_EXACT>(s, v, end, 0, cfg, end, false, false, &e);
        break;
    }
    default: break;                                // arrays and ext values have no ra value: nothing is added
    }
}

// the spans of a captured row: [column][emitted row]
struct RtSpans {
    const uint32_t *base;
    uint64_t n, e;
    DEV uint32_t get(uint32_t col) const { return base ? base[(uint64_t) col * n + e] : CAP_UNSET; }
};

// flb_ra_translate (src/flb_record_accessor.c:644-699) of rule ri's NEW_TAG into s.  val: the matched value (the text the spans index)
template <class S>
DEV void rt_compose(const RtagArgs &a, const RtTable &tb, uint32_t ri, const uint8_t *body, const uint8_t *end, const uint8_t *val, uint32_t vlen,
                    const RtSpans &sp, int ngroups, S &s) {
    const LDS_AS uint32_t *r = tb.w + RT_RULE_WORDS * ri;
    const uint32_t nparts = (r[0] >> 16) & 0xffu;
    const LDS_AS uint32_t *pt = tb.w + (r[4] >> 2);
    for (uint32_t k = 0; k < nparts; k++, pt += RT_PART_WORDS) {
        const uint32_t kind = pt[0] & 0xffu;
        if (kind == RT_P_STR) { for (uint32_t j = 0; j < pt[1]; j++) s.put((tb.w[(pt[2] >> 2) + (j >> 2)] >> (8 * (j & 3))) & 0xffu); }
        else if (kind == RT_P_TAG) s.copy(a.tag, a.tag_len);
        else if (kind == RT_P_TAGPART) rt_tag_part(s, a.tag, a.tag_len, (int32_t) pt[1]);
        else if (kind == RT_P_REGEX) {
            // flb_regex_results_get: no region (a pattern without groups), an id past the registers, or an unset group add nothing
            const uint32_t g = pt[1];
            if (ngroups <= 0 || g > (uint32_t) ngroups || g > 9) continue;
            const uint32_t b = sp.get(2 * g), e = sp.get(2 * g + 1);
            if (b == CAP_UNSET || e == CAP_UNSET || b > e || e > vlen) continue;
            s.copy(val + b, e - b);
        }
        else {
            const uint8_t *v = ra_lds_path(tb.w, tb.w + (pt[2] >> 2), pt[1], tb.w + (pt[3] >> 2), (pt[0] >> 8) & 0xffu, body, end, true);
            if (v) rt_value(s, v, end);
        }
    }
}

__global__ void __launch_bounds__(RT_BLOCK) k_rtag_match(RtagArgs a) {
    RtTable tb{lane_stage_table<RT_BLOCK>(a.table, a.table_bytes), a.nrules};
    __syncthreads();
    const uint64_t gsz = (uint64_t) gridDim.x * RT_BLOCK;
    unsigned long long n_dec = 0, n_keep = 0, n_match = 0, n_big = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * RT_BLOCK + threadIdx.x; r < a.n; r += gsz) {
        const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
        uint32_t rule = RT_ROW_SKIP, keep = 0, emit = 0;
        if (rec != end) {
            Event ev = decode_event(rec, end);
            if ((ev.flags & RF_BAD) || ev.body_end != end) { atomicMin(a.first_bad, (unsigned long long) r); rule = RT_ROW_NONE; }
            else if (!(ev.flags & RF_SKIP)) {
                n_dec++;
                rule = RT_ROW_NONE;
                for (uint32_t ri = 0; ri < (uint32_t) a.nrules; ri++) {
                    uint32_t vlen = 0;
                    const uint8_t *val = rt_key_value(tb, ri, ev.body, end, vlen);
                    if (val && rt_match(a.rules[ri], val, vlen)) { rule = ri; break; }
                }
                const uint64_t len = (uint64_t) (end - rec);
                if (len > 0xFFFFFFFFull) { n_big++; rule = RT_ROW_NONE; }
                else {
                    if (rule != RT_ROW_NONE) { emit = 1; n_match++; }
                    if (rule == RT_ROW_NONE || (tb.w[RT_RULE_WORDS * rule] & RT_KEEP)) { keep = (uint32_t) len; n_keep++; }
                }
            }
        }
        a.rule[r] = rule; a.keep_len[r] = keep; a.emit[r] = emit;
    }
    n_dec = lane_wave_sum(n_dec); n_keep = lane_wave_sum(n_keep); n_match = lane_wave_sum(n_match); n_big = lane_wave_sum(n_big);
    if ((threadIdx.x & 63u) == 0) {
        if (n_dec) atomicAdd(&a.counts[0], n_dec);
        if (n_keep) atomicAdd(&a.counts[1], n_keep);
        if (n_match) atomicAdd(&a.counts[2], n_match);
        if (n_big) atomicAdd(&a.counts[3], n_big);
    }
}

// the emitted rows: EMIT false sizes the tag (after the capture walk where the template needs one), EMIT true writes it and the row's
// entry of the emitted table.  A wave keeps its own part of the capture scratch for the whole launch.
template <bool EMIT>
__global__ void __launch_bounds__(RT_BLOCK) k_rtag(RtagArgs a) {
    RtTable tb{lane_stage_table<RT_BLOCK>(a.table, a.table_bytes), a.nrules};
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave_slot = ((uint64_t) blockIdx.x * RT_BLOCK + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t) gridDim.x * RT_BLOCK) >> 6;
    uint16_t *chk = a.chk ? a.chk + ((size_t) wave_slot * a.chk_len) * 64 + lane : nullptr;
    unsigned long long n_mis = 0, n_big = 0, n_bytes = 0;
    for (uint64_t base = wave_slot * 64; base < a.n; base += nwaves * 64) {
        const uint64_t r = base + lane;
        if (r >= a.n) continue;
        if (!a.emit[r]) { if (!EMIT) a.tag_lens[r] = 0; continue; }
        const uint32_t ri = a.rule[r];
        const uint64_t e = a.emit_idx[r];
        const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
        uint32_t vlen = 0;
        const uint8_t *val = nullptr, *body = nullptr;
        bool ok = ri < (uint32_t) a.nrules && e < a.n_emit;
        if (ok) {
            Event ev = decode_event(rec, end);
            ok = !(ev.flags & (RF_BAD | RF_SKIP)) && ev.body_end == end;
            body = ev.body;
            if (ok) { val = rt_key_value(tb, ri, body, end, vlen); ok = val != nullptr; }
        }
        if (!ok) { n_mis++; if (!EMIT) a.tag_lens[r] = 0; continue; }
        const uint32_t r0 = tb.w[RT_RULE_WORDS * ri];
        const bool cap = (r0 & RT_NEEDS_CAP) != 0;
        int ngroups = 0;
        if (cap) {
            const RtagCap &pc = a.caps[tb.w[RT_RULE_WORDS * ri + 5]];
            ngroups = pc.ngroups;
            if (!EMIT) {
                CapGlobal cg;
                cg.base = a.spans; cg.n = a.n_emit; cg.r = e;
                for (uint32_t f = 0; f < RT_CAP_COLS; f++) cg.set(f, CAP_UNSET);
                if (!chk || !rt_capture(pc, val, vlen, chk, a.chk_len, a.chk_nfa_off, cg)) {
                    n_mis++;
                    for (uint32_t f = 0; f < RT_CAP_COLS; f++) cg.set(f, CAP_UNSET);
                }
            }
        }
        RtSpans sp{cap ? a.spans : nullptr, a.n_emit, e};
        if (!EMIT) {
            CountSink cs;
            rt_compose(a, tb, ri, body, end, val, vlen, sp, ngroups, cs);
            if (cs.n > 0xFFFFFFFFull) { n_big++; cs.n = 0; }
            a.tag_lens[r] = (uint32_t) cs.n;
            continue;
        }
        uint8_t *t0 = a.tags + a.tag_off[r], *t1 = a.tags + a.tag_off[r + 1];
        RtSink bs(t0, t1);
        rt_compose(a, tb, ri, body, end, val, vlen, sp, ngroups, bs);
        if (bs.over || bs.p != t1) n_mis++;
        n_bytes += (unsigned long long) (t1 - t0);
        // data + pre (rewrite_tag.c:494): from the end of the record the decoder handed out before this one -- the rows in between
        // (group markers, records an earlier filter dropped) travel with it
        uint64_t s0 = r;
        while (s0 > 0 && a.rule[s0 - 1] == RT_ROW_SKIP) s0--;
        const uint64_t in_off = a.row_off[s0], in_len = a.row_off[r + 1] - in_off;
        if (in_len > 0xFFFFFFFFull) n_big++;
        RtagEmitted o;
        o.in_off = in_off; o.tag_off = a.tag_off[r]; o.len = (uint32_t) in_len; o.tag_len = (uint32_t) (t1 - t0);
        a.table_out[e] = o;
    }
    // one atomic per wave and counter that is not zero (every lane of the wave is here again behind the loop)
    n_mis = lane_wave_sum(n_mis); n_big = lane_wave_sum(n_big); n_bytes = lane_wave_sum(n_bytes);
    if (lane == 0) {
        if (n_mis) atomicAdd(&a.counts[4], n_mis);
        if (n_big) atomicAdd(&a.counts[3], n_big);
        if (EMIT && n_bytes) atomicAdd(&a.counts[5], n_bytes);
    }
}

// a refused emission keeps its record (rewrite_tag.c:417-420)
__global__ void __launch_bounds__(RT_BLOCK) k_rtag_refuse(RtagArgs a, const uint32_t *refused) {
    const uint64_t gsz = (uint64_t) gridDim.x * RT_BLOCK;
    for (uint64_t r = (uint64_t) blockIdx.x * RT_BLOCK + threadIdx.x; r < a.n; r += gsz) {
        if (!a.emit[r]) continue;
        const uint64_t e = a.emit_idx[r];
        if (e < a.n_emit && ((refused[e >> 5] >> (e & 31)) & 1u)) a.keep_len[r] = (uint32_t) (a.row_off[r + 1] - a.row_off[r]);
    }
}

void launch_rtag_match(const RtagArgs &a, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_rtag_match, dim3(lane_blocks<RT_BLOCK>(a.n)), dim3(RT_BLOCK), a.table_bytes, st, a);
}

// waves: how many the capture scratch has room for (a multiple of RT_BLOCK / 64)
void launch_rtag(const RtagArgs &a, bool emit, int waves, hipStream_t st) {
    if (a.n == 0) return;
    unsigned blocks = lane_blocks<RT_BLOCK>(a.n);
    const unsigned cap = (unsigned) (waves / (RT_BLOCK / 64));
    if (cap >= 1 && blocks > cap) blocks = cap;
    if (emit) hipLaunchKernelGGL(k_rtag<true>, dim3(blocks), dim3(RT_BLOCK), a.table_bytes, st, a);
    else hipLaunchKernelGGL(k_rtag<false>, dim3(blocks), dim3(RT_BLOCK), a.table_bytes, st, a);
}

void launch_rtag_refuse(const RtagArgs &a, const uint32_t *refused, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_rtag_refuse, dim3(lane_blocks<RT_BLOCK>(a.n)), dim3(RT_BLOCK), 0, st, a, refused);
}
