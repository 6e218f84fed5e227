// typeconv_kernels.inc -- filter_type_converter (plugins/filter_type_converter/type_converter.c:182-353, src/flb_typecast.c): a lane
// per record.  ONE function, tc_record, writes a record into whatever sink it is given: the size pass hands it a CountSink, the emit
// pass a BoundedSink that never stores outside the row's own [out_off[r], out_off[r + 1]).  Both passes therefore walk the same code; a
// row whose emitted length is not its sized length (or that ran into the end of its room) is counted, not written past.  The
// original entries go out as put_entries re-packs them (runs of already-canonical entries as one span); behind them, for every
// rule whose key the ORIGINAL body holds, to_key and the converted value -- or the value as it was when the conversion fails.
// Nested values are never interpreted, only walked; the numbers come from numconv.hpp and write straight into the sink.
// Included inside namespace flbgpu after kdev.inc, lane_rows.inc, canon_walk.inc (the sinks' helpers) and ra_lds.inc (the key lookup).

struct TcTable {
    const LDS_AS uint32_t *w;       // the table's words in LDS
    int nrules;
};

// flb_ra_get_kv_pair (src/flb_record_accessor.c:788-801, src/flb_ra_key.c:151-236, 374-434) on the original body (ra_lds.inc).  A
// path that ends on an array index has no key object, and the filter reads that as "not found" (type_converter.c:277-281).
DEV const uint8_t *tc_lookup(const TcTable &tb, int ri, const uint8_t *body, const uint8_t *end) {
    const LDS_AS uint32_t *r = tb.w + TC_RULE_WORDS * (uint32_t) ri;
    if (r[0] & TC_INERT) return nullptr;
    return ra_lds_path(tb.w, tb.w + (r[2] >> 2), r[1], tb.w + (r[5] >> 2), (r[0] >> 16) & 0xffu, body, end, false);
}

struct TcSrc {
    const uint8_t *p;
    uint32_t n;
    DEV uint32_t operator[](uint32_t i) const { return i < n ? ld8(p + i) : 0u; }
};
struct TcDigits { uint32_t n = 0; DEV void put(uint32_t) { n++; } };
template <class S> struct TcDst { S &s; DEV void put(uint32_t c) { s.put(c); } };

template <class S> DEV void tc_f64(S &s, uint64_t bits) { s.put(0xcb); pk_be(s, bits, 8); }

// flb_typecast_pack (src/flb_typecast.c:396-457, 72-341) of the value at v under rule word r0: true when the converted value was
// written, false when nothing was (the caller writes the value as it is)
template <class S> DEV bool tc_convert(uint32_t r0, const uint8_t *v, const uint8_t *end, S &s, bool &undef) {
    const uint32_t src = r0 & 0xffu, to = (r0 >> 8) & 0xffu;
    Tok t = mp_tok(v, end);
    if (src == TC_SRC_STR) {
        if (t.type != T_STR) return false;
        TcSrc in{t.next, t.len};
        switch (to) {
        case TC_TO_INT: {
            const uint64_t x = nc::scan_intmax(in, t.len, 10, true);
            if (x == 0) return false;
            pk_int(s, (int64_t) x);
            return true;
        }
        case TC_TO_UINT: case TC_TO_HEX: {
            const uint64_t x = nc::scan_intmax(in, t.len, to == TC_TO_HEX ? 16u : 10u, false);
            if (x == 0) return false;
            pk_uint(s, x);
            return true;
        }
        case TC_TO_FLOAT: {
            const nc::ScanResult sr = nc::scan_double<true>(in, t.len, nc::MODE_STRTOD | nc::MODE_NAN_PAYLOAD);
            tc_f64(s, sr.status == nc::NC_OK ? sr.bits : 0);          // atof: no conversion is 0.0
            return true;
        }
        case TC_TO_BOOL: {
            const uint32_t c0 = nc::lower(in[0]), c1 = nc::lower(in[1]), c2 = nc::lower(in[2]), c3 = nc::lower(in[3]), c4 = nc::lower(in[4]);
            if (t.len >= 4 && c0 == 't' && c1 == 'r' && c2 == 'u' && c3 == 'e') { s.put(0xc3); return true; }
            if (t.len >= 5 && c0 == 'f' && c1 == 'a' && c2 == 'l' && c3 == 's' && c4 == 'e') { s.put(0xc2); return true; }
            return false;
        }
        default: return false;
        }
    }
    if (src == TC_SRC_INT || src == TC_SRC_UINT) {
        if (t.type != T_UINT && t.type != T_NINT) return false;
        const bool sgn = src == TC_SRC_INT;
        switch (to) {
        case TC_TO_STR: {
            TcDigits d;
            if (sgn) nc::fmt_ld((int64_t) t.u, d); else nc::fmt_lu(t.u, d);
            pk_str_hdr(s, d.n);
            TcDst<S> o{s};
            if (sgn) nc::fmt_ld((int64_t) t.u, o); else nc::fmt_lu(t.u, o);
            return true;
        }
        case TC_TO_FLOAT: tc_f64(s, sgn ? nc::i64_to_double_bits((int64_t) t.u) : nc::u64_to_double_bits(t.u)); return true;
        case TC_TO_UINT: if (!sgn) return false; pk_uint(s, t.u); return true;
        case TC_TO_INT: if (sgn) return false; pk_int(s, (int64_t) t.u); return true;
        default: return false;
        }
    }
    if (t.type != T_F32 && t.type != T_F64) return false;
    const uint64_t bits = t.type == T_F64 ? t.u : (uint64_t) __double_as_longlong((double) __uint_as_float((uint32_t) t.u));
    switch (to) {
    case TC_TO_STR: {
        TcDigits d;
        nc::fmt_json_double(bits, false, d);
        pk_str_hdr(s, d.n);
        TcDst<S> o{s};
        nc::fmt_json_double(bits, false, o);
        return true;
    }
    case TC_TO_INT: pk_int(s, (int64_t) nc::double_to_i64_x86(bits, undef)); return true;
    case TC_TO_UINT: pk_uint(s, nc::double_to_u64_x86(bits, undef)); return true;
    default: return false;
    }
}

struct TcRow {
    bool bad, decoded;
    uint32_t done, failed, undef;
    uint64_t len;                       // output bytes (0: nothing emitted)
};

// one record of the loop (:240-318) into s; false: the row is not one well-formed event
template <class S> DEV bool tc_record(const TcTable &tb, const Event &ev, const uint8_t *end, S &s, TcRow &w) {
    uint32_t sec, nsec;
    event_time_or_zero(ev, sec, nsec);                                // (its answer is overwritten, :252-257)
    put_event_head(s, sec, nsec);
    put_meta(s, ev);
    uint8_t *hdr = open_map32(s);
    Tok bm = mp_tok(ev.body, end);
    // the original entries, in order
    if (!put_entries(s, bm, end, [](uint32_t, const uint8_t *, const uint8_t *) { return ENTRY_KEEP; })) return false;
    uint64_t found = 0;
    for (int ri = 0; ri < tb.nrules; ri++) {
        const uint8_t *v = tc_lookup(tb, ri, ev.body, end);
        if (!v) continue;
        found++;
        const LDS_AS uint32_t *r = tb.w + TC_RULE_WORDS * (uint32_t) ri;
        put_lds(s, tb.w + (r[4] >> 2), r[3]);
        bool undef = false;
        if (tc_convert(r[0], v, end, s, undef)) { w.done++; w.undef += undef ? 1u : 0u; }
        else { w.failed++; mp_canon(v, end, s, 2); }
    }
    close_map32(s, hdr, (uint64_t) bm.len + found);
    return true;
}

// size pass: rows an earlier filter dropped, group markers and decoder errors as rm_size treats them
DEV TcRow tc_size(const TypeconvArgs &a, const TcTable &tb, uint64_t r) {
    TcRow w;
    w.bad = false; w.decoded = false; w.done = 0; w.failed = 0; w.undef = 0; w.len = 0;
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    if (rec == end) return w;                                         // a record an earlier filter dropped
    Event ev = decode_event(rec, end, true);
    if (ev.flags & RF_BAD) { w.bad = true; return w; }
    CountSink cs;
    if (!tc_record(tb, ev, end, cs, w)) { w.bad = true; w.done = 0; w.failed = 0; w.undef = 0; return w; }
    if (ev.flags & RF_SKIP) { w.done = 0; w.failed = 0; w.undef = 0; return w; }      // group markers: skipped by the decoder
    w.decoded = true;
    w.len = cs.n;
    return w;
}

// emit pass: the record whose length the size pass wrote, into its own room and no further; true: the lengths agree
DEV bool tc_emit(const TypeconvArgs &a, const TcTable &tb, uint64_t r) {
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    Event ev = decode_event(rec, end, true);
    if (ev.flags & RF_BAD) return false;
    uint8_t *o0 = a.out + a.out_off[r], *o1 = a.out + a.out_off[r + 1];
    BoundedSink bs(o0, o1);
    TcRow w;
    w.bad = false; w.decoded = false; w.done = 0; w.failed = 0; w.undef = 0; w.len = 0;
    const bool ok = tc_record(tb, ev, end, bs, w);
    return ok && !bs.over && bs.p == o1;
}

template <bool EMIT>
__global__ void __launch_bounds__(TC_BLOCK) k_typeconv(TypeconvArgs a) {
    TcTable tb{lane_stage_table<TC_BLOCK>(a.table, a.table_bytes), a.nrules};
    __syncthreads();
    unsigned long long n_dec = 0, n_out = 0, n_done = 0, n_failed = 0, n_undef = 0, n_big = 0, n_mis = 0;
    lane_wave_rows<TC_BLOCK>(a.n, [&](uint64_t r, bool live) {
        if (EMIT) {
            if (live && a.len[r] && !tc_emit(a, tb, r)) n_mis++;
            return;
        }
        TcRow w;
        w.bad = false; w.decoded = false; w.done = 0; w.failed = 0; w.undef = 0; w.len = 0;
        if (live) {
            w = tc_size(a, tb, r);
            const bool big = w.len > 0xFFFFFFFFull;                    // a row the u32 length column cannot hold
            if (big) { n_big++; w.len = 0; }
            a.len[r] = (uint32_t) w.len;
            n_done += w.done; n_failed += w.failed; n_undef += w.undef;
            if (w.bad) atomicMin(a.first_bad, (unsigned long long) r);
        }
        lane_count(n_dec, w.decoded); lane_count(n_out, w.len != 0);
    });
    if (EMIT) { lane_flush(&a.counts[6], n_mis); return; }
    // one atomic per wave and counter that is not zero (every lane of the wave is here: the loop's trip count is the wave's)
    n_done = lane_wave_sum(n_done); n_failed = lane_wave_sum(n_failed); n_undef = lane_wave_sum(n_undef);
    lane_flush(&a.counts[0], n_dec); lane_flush(&a.counts[1], n_out);                                         // (lane 0's)
    if ((threadIdx.x & 63u) == 0) { lane_flush(&a.counts[2], n_done); lane_flush(&a.counts[3], n_failed); lane_flush(&a.counts[4], n_undef); }
    lane_flush(&a.counts[5], n_big);
}

void launch_typeconv(const TypeconvArgs &a, bool emit, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 g(lane_blocks<TC_BLOCK>(a.n)), b(TC_BLOCK);
    if (emit) hipLaunchKernelGGL(k_typeconv<true>, g, b, a.table_bytes, st, a);
    else hipLaunchKernelGGL(k_typeconv<false>, g, b, a.table_bytes, st, a);
}
