// dec_dev.inc -- a parser's Decode_Field / Decode_Field_As rules on the device (src/flb_parser_decoder.c:215-550).
//
// The reference applies them to the msgpack map a parser has packed (regex / logfmt / ltsv: after the parser's own time handling,
// src/flb_parser_regex.c:210-221, flb_parser_logfmt.c:314-324, flb_parser_ltsv.c:257-267; Format json: BEFORE its time lookup,
// src/flb_parser_json.c:100-114) and filter_parser then works with the new map.  The device version keeps that shape instead of
// threading the rules through the three fast record writers: for a record whose winning parser has decoders, one lane
//   1. packs the parser's map into its scratch (the same field / pair writers the emit kernels use, into a memory sink),
//   2. runs the rule engine over that map: key match in map order, one Decode_Field and one Decode_Field_As per key, try_next /
//      do_next, the four backends (json through the wide JSON walker, the string ones through csrc/dec.hpp), the extra keys of
//      the LAST Decode_Field key merged behind the map (first decoded object only: merge_record_and_extra_keys :149-209),
//   3. Format json: looks the time key up in the DECODED map and re-packs the map without it (flb_parser_json.c:116-233),
//   4. writes the record: event header, metadata, the map (+ what Reserve_Data / Preserve_Key append).
// It runs twice (CountSink for the size pass, ByteSink for the emit pass: k_parser_dec); rows it owns carry RF_DEC and are left
// alone by k_parser_emit.  Everything here is the slow, exact path: decoders are a per-record rewrite of strings into objects,
// not a scan.  Scratch per lane: DEC_REGIONS regions of `cap` bytes (map A, map B, two text halves, the Decode_Field object,
// the extra-keys buffer; the merged map goes back into region 0); a row whose region overflows in the size pass is counted
// (DecArgs::err) and the host runs the size pass again with twice the room before it uses any size (flbgpu.cpp run_parser_dev: the
// first cap is a guess from the chunk's longest record, 2.25 to 4.5 bytes per byte of text are ordinary for short JSON numbers).
// (csrc/dec.hpp -- the string backends, one template for host and device -- is included by the translation unit, outside the namespace)

struct MemSink {
    uint8_t *p, *limit;
    bool ovf = false;
    DEV MemSink(uint8_t *b, uint8_t *l) : p(b), limit(l) {}
    DEV void note_exact() {}
    DEV void put(uint32_t b) { if (p < limit) *p = (uint8_t) b; else ovf = true; p++; }
    DEV void copy(const uint8_t *src, uint32_t len) {
        if (p + len <= limit) for (uint32_t i = 0; i < len; i++) p[i] = (uint8_t) ld8(src + i);
        else ovf = true;
        p += len;
    }
    DEV void words(const uint32_t *w, uint32_t nbytes) { for (uint32_t i = 0; i < nbytes; i++) put((w[i >> 2] >> (8 * (i & 3))) & 255u); }
    DEV void put32(uint32_t v) { put(v & 255u); put((v >> 8) & 255u); put((v >> 16) & 255u); put(v >> 24); }
    DEV void put16(const v4u32 w, uint32_t nbytes) { for (uint32_t i = 0; i < nbytes; i++) put(v4_byte(w, i)); }
    DEV void finish() {}
};
// the text a backend works on: the reference hands it an sds copy -- byte n is the terminating NUL
struct MemSrc {
    const uint8_t *p;
    uint32_t n;
    DEV uint32_t operator[](uint32_t i) const { return i < n ? ld8(p + i) : 0u; }
};

DEV bool dec_key_is(const DevDecoder &d, const uint8_t *k, uint32_t klen) {
    if (d.key_len != klen) return false;
    for (uint32_t i = 0; i < klen; i++) if (ld8(k + i) != d.key[i]) return false;
    return true;
}

// decode_json (:38-86): leading blanks, '{' or '[' must follow, flb_pack_json_recs of the rest: exactly ONE record, an object
template <class S> DEV bool dec_backend_json(const uint8_t *data, uint32_t n, S &o) {
    MemSrc in{data, n};
    uint32_t p = 0;
    while (in[p] == ' ') p++;
    if (in[p] != '{' && in[p] != '[') return false;
    JsonSrc s;
    s.p = data + p; s.len = n - p;
    JsonCounts cc;
    cc.col = nullptr; cc.n = 0; cc.r = 0; cc.store = false; cc.next = JSON_CNT_SLOTS;       // (no cached container counts: count as you go)
    uint32_t pos = 0, nrec = 0;
    int root = 0, status = JS_OK;
    while (pos < s.len) {
        while (pos < s.len && js_ws(s[pos])) pos++;
        if (pos >= s.len) break;
        int rt = 0;
        uint32_t e;
        if (nrec == 0) e = js_value<true, JSON_GENERIC_WORDS>(s, pos, o, rt, status, cc);
        else { JsonNullSink ns; e = js_value<true, JSON_GENERIC_WORDS>(s, pos, ns, rt, status, cc); }
        if (status != JS_OK) return false;
        if (!e) break;                                      // the first value that fails ends the stream
        if (nrec == 0) root = rt;
        nrec++;
        pos = e;
    }
    return nrec == 1 && root == 1;                          // (1 = object: flb_pack.h FLB_PACK_JSON_OBJECT / JSMN_OBJECT)
}

// one backend on the current text; *dtype: 0 a string, 1 a packed object
template <class S> DEV bool dec_backend(uint32_t backend, const uint8_t *data, uint32_t n, S &o, int *dtype) {
    MemSrc in{data, n};
    *dtype = 0;
    switch (backend) {
    case dec::BK_JSON: *dtype = 1; return dec_backend_json(data, n, o);
    case dec::BK_ESCAPED: dec::unescape_plain(in, n, o); return true;
    case dec::BK_ESCAPED_UTF8: dec::unescape_utf8<false>(in, n, o); return true;
    default: dec::mysql_quoted(in, n, o); return true;
    }
}

// flb_parser_decoder_do on the map [m, m_end).  false: no key of the map has a decoder (the map stays as it is); true: the new map
// is [*out, *out_end) inside the scratch.  rg: the lane's DEC_REGIONS regions of `cap` bytes; region 0 holds the input map.
DEV bool dec_apply(const DevDecoders &D, const uint8_t *m, const uint8_t *m_end, uint8_t *rg, uint32_t cap, const uint8_t **out, const uint8_t **out_end,
                   bool &ovf) {
    const Tok mh = mp_tok(m, m_end);
    if (mh.type != T_MAP) return false;
    int matched = -1;
    {
        const uint8_t *p = mh.next;
        for (uint32_t i = 0; i < mh.len && matched < 0; i++) {
            const Tok k = mp_tok(p, m_end);
            const uint8_t *kend = mp_end_of(k, p, m_end);
            if (!kend) return false;
            if (k.type == T_STR) for (uint32_t q = 0; q < D.n; q++) if (dec_key_is(D.d[q], k.next, k.len)) { matched = (int) i; break; }
            const uint8_t *vend = mp_skip(kend, m_end);
            if (!vend) return false;
            p = vend;
        }
    }
    if (matched < 0) return false;
    uint8_t *B = rg + (size_t) cap, *T0 = rg + 2 * (size_t) cap, *T1 = rg + 3 * (size_t) cap, *O = rg + 4 * (size_t) cap, *E = rg + 5 * (size_t) cap;
    MemSink b(B, B + cap);
    pk_map_hdr(b, mh.len);
    bool extra_keys = false;
    uint32_t e_len = 0;
    const uint8_t *p = mh.next;
    for (uint32_t i = 0; i < mh.len; i++) {
        const Tok k = mp_tok(p, m_end);
        const uint8_t *kend = mp_end_of(k, p, m_end);
        const Tok v = mp_tok(kend, m_end);
        const uint8_t *vend = mp_end_of(v, kend, m_end);
        const DevDecoder *dc = nullptr;
        if ((int) i >= matched && k.type == T_STR && v.type == T_STR)
            for (uint32_t q = 0; q < D.n; q++) if (dec_key_is(D.d[q], k.next, k.len)) { dc = &D.d[q]; break; }
        if (!dc) { mp_canon(p, m_end, b); mp_canon(kend, m_end, b); p = vend; continue; }
        const uint8_t *data = v.next, *in_ptr = nullptr;
        uint32_t data_len = v.len, in_len = 0, out_len = 0;
        int in_type = 0, out_type = 0;
        bool is_decoded = false, is_decoded_as = false;
        uint32_t tsel = 0;
        if (dc->add_extra_keys) { extra_keys = true; e_len = 0; }        // (the buffer of an earlier key is dropped: :404-412)
        for (uint32_t ri = 0; ri < dc->nrules; ri++) {
            const DevDecRule rule = dc->rules[ri];
            if (rule.type == DEC_T_DEFAULT && rule.action == DEC_A_DO_NEXT && is_decoded) continue;
            if (is_decoded_as && in_type != 0) continue;
            uint8_t *dst = tsel ? T1 : T0;
            MemSink ds(dst, dst + cap);
            int dtype = 0;
            if (!dec_backend(rule.backend, data, data_len, ds, &dtype)) {
                if (rule.action == DEC_A_TRY_NEXT || rule.action == DEC_A_DO_NEXT) continue;
                break;
            }
            if (ds.ovf) { ovf = true; return false; }
            const uint32_t dsize = (uint32_t) (ds.p - dst);
            if (rule.type == DEC_T_AS) {
                in_ptr = dst; in_len = dsize; data = dst; data_len = dsize; in_type = dtype; is_decoded_as = true;
                tsel ^= 1;                                           // the next backend reads this half and writes the other
            }
            else {
                for (uint32_t q = 0; q < dsize; q++) O[q] = dst[q];  // out_sds: the last successful Decode_Field of the key
                out_len = dsize; out_type = dtype; is_decoded = true;
            }
            if (rule.action == DEC_A_DO_NEXT) continue;
            break;
        }
        mp_canon(p, m_end, b);                                       // the key
        if (is_decoded_as) {
            if (in_type == 0) { pk_str_hdr(b, in_len); b.copy(in_ptr, in_len); }
            else b.copy(in_ptr, in_len);
        }
        else mp_canon(kend, m_end, b);
        if (is_decoded && out_type == 1) {                           // (a string: "not allowed", logged only :506-508)
            if (e_len + out_len > cap) { ovf = true; return false; }
            for (uint32_t q = 0; q < out_len; q++) E[e_len + q] = O[q];
            e_len += out_len;
        }
        p = vend;
    }
    if (b.ovf) { ovf = true; return false; }
    *out = B; *out_end = b.p;
    if (extra_keys && e_len > 0) {
        // merge_record_and_extra_keys: the FIRST object of the extra buffer behind the record's pairs, one map header for both
        const Tok eh = mp_tok(E, E + e_len);
        const uint8_t *e_end = mp_skip(E, E + e_len);
        const Tok bh = mp_tok(B, b.p);
        if (eh.type == T_MAP && e_end && bh.type == T_MAP) {
            MemSink a(rg, rg + cap);                                 // (the input map is not needed any more)
            pk_map_hdr(a, bh.len + eh.len);
            const uint8_t *q = bh.next;
            for (uint32_t i = 0; i < 2 * bh.len; i++) q = mp_canon(q, b.p, a);
            q = eh.next;
            for (uint32_t i = 0; i < 2 * eh.len; i++) q = mp_canon(q, e_end, a);
            if (a.ovf) { ovf = true; return false; }
            *out = rg; *out_end = a.p;
        }
    }
    return true;
}

// The complete output record of row `ri` whose winning parser has decoders.  *sec / *nsec: the record's timestamp (in: what the
// size pass settled; out: Format json may have found another one in the decoded map).  Returns false when the scratch overflowed.
template <class S, class CV>
DEV bool dec_record(S &s, const FParserCfg &cfg, const DevParser *parsers, const uint8_t *rec, const uint8_t *rec_end, const RecInfo &ri, const CV &caps,
                    uint64_t null_mask, uint8_t *rg, uint32_t cap, int64_t *sec, int64_t *nsec, bool *badts) {
    const DevParser &ps = parsers[ri.parser_idx];
    const uint8_t *val = rec + ri.val_off;
    *badts = false;
    // ---- 1. the parser's map
    MemSink a(rg, rg + cap);
    const bool json_fmt = ps.is_json && !ps.kv_format;
    if (json_fmt) {
        JsonSrc js;
        js.p = val; js.len = ri.val_len;
        JsonCounts cc;
        cc.col = nullptr; cc.n = 0; cc.r = 0; cc.store = false; cc.next = JSON_CNT_SLOTS;
        uint32_t pos = 0;
        while (pos < js.len && js_ws(js[pos])) pos++;
        int rt = 0, status = JS_OK;
        js_value<true, JSON_GENERIC_WORDS>(js, pos, a, rt, status, cc);
    }
    else if (ps.kv_format) {
        pk_map_hdr(a, ri.nkept);
        pkv_emit_pairs<true>(ps, val, ri.val_len, a);
    }
    else {
        // header patched in place: width of the ORIGINAL count is kept (flb_parser_regex.c:182-199)
        const uint32_t n0 = (uint32_t) ps.nregs_minus1;
        if (n0 < 16) a.put(0x80 | ri.nkept);
        else if (n0 < 65536) { a.put(0xde); pk_be(a, ri.nkept, 2); }
        else { a.put(0xdf); pk_be(a, ri.nkept, 4); }
        for (int f = 0; f < ps.nfields; f++) {
            if ((ri.drop_mask >> f) & 1) continue;
            const uint32_t b = caps[2 * f], e = caps[2 * f + 1];
            const uint32_t vlen = (b == CAP_UNSET || e == CAP_UNSET) ? 0 : e - b;
            const uint8_t *v = (b == CAP_UNSET || e == CAP_UNSET) ? val : val + b;
            a.words(ps.keywords + ps.kw_off[f], (uint32_t) ps.kw_bytes[f]);
            write_field_value<true>(a, ps.field_type[f], v, vlen);
        }
    }
    if (a.ovf) return false;
    // ---- 2. the decoders
    const uint8_t *m = rg, *m_end = a.p;
    bool ovf = false;
    bool canonical_hdr = json_fmt || ps.kv_format != 0;
    {
        const uint8_t *o = nullptr, *oe = nullptr;
        if (dec_apply(*ps.decs, m, m_end, rg, cap, &o, &oe, ovf)) { m = o; m_end = oe; canonical_hdr = true; }
        if (ovf) return false;
    }
    // ---- 3. Format json: the time key of the decoded map (flb_parser_json.c:116-233)
    uint32_t skip = 0xFFFFFFFFu;
    bool repack = false;
    if (json_fmt) {
        Event ev = decode_event(rec, rec_end, true);
        int64_t tsec = ev.sec, tnsec = ev.nsec;
        if (ps.has_time) {
            const Tok mh = mp_tok(m, m_end);
            const uint8_t *p = mh.next;
            for (uint32_t i = 0; i < mh.len; i++) {
                const Tok k = mp_tok(p, m_end);
                const uint8_t *kend = mp_end_of(k, p, m_end);
                const Tok v = mp_tok(kend, m_end);
                const uint8_t *vend = mp_end_of(v, kend, m_end);
                bool hit = k.type == T_STR && k.len == (uint32_t) ps.tkey_len;
                for (uint32_t q = 0; hit && q < k.len; q++) hit = ld8(k.next + q) == (uint8_t) ps.tkey[q];
                if (hit) {
                    if (v.type == T_STR) {
                        int64_t s2 = 0;
                        double frac = 0;
                        repack = true;
                        if (time_lookup(ps, v.next, v.len, &s2, &frac) == 0) {
                            if (!ps.time_keep) skip = i;
                            const int64_t ns2 = (int64_t) (frac * 1000000000.0);
                            if ((uint64_t) s2 * 1000000000ull + (uint64_t) ns2 != 0) { tsec = s2; tnsec = ns2; }
                        }
                    }
                    break;
                }
                p = vend;
            }
        }
        if (encoder_refuses_time(tsec, tnsec)) { *badts = true; return true; }
        *sec = tsec; *nsec = tnsec;
    }
    // ---- 4. the record
    s.put32(0x00d79292u); s.put32(__builtin_bswap32((uint32_t) *sec)); s.put32(__builtin_bswap32((uint32_t) *nsec));
    if (ri.meta_len > 1) mp_canon(rec + ri.meta_off, rec + ri.meta_off + ri.meta_len, s);
    else s.put(0x80);
    const uint8_t *body = rec + ri.body_off, *body_end = body + ri.body_len;
    Tok bm;
    bm.type = T_MAP; bm.len = 0; bm.u = 0; bm.next = body;
    uint32_t nappend = 0;
    const bool plain_key = !cfg.key.is_ra;
    if (cfg.reserve_data || cfg.preserve_key) bm = mp_tok(body, body_end);
    if (cfg.reserve_data) {
        nappend = bm.len;
        if (plain_key && !cfg.preserve_key) {
            for (uint32_t i = 0; i < bm.len && i < 64; i++) if ((null_mask >> i) & 1) nappend--;
            if (bm.len > 64) nappend -= null_count_high(cfg, caps.r);
        }
    }
    else if (cfg.preserve_key && plain_key) nappend = 1;
    const Tok mh = mp_tok(m, m_end);
    const uint32_t npairs = mh.len - (skip != 0xFFFFFFFFu ? 1u : 0u);
    if (nappend > 0 || repack || !canonical_hdr) {
        // flb_msgpack_expand_map / the json parser's re-pack: one canonical header, every pair re-packed
        if (nappend > 0 || repack) pk_map_hdr(s, npairs + nappend);
        else s.copy(m, (uint32_t) (mh.next - m));                    // (the regex parser's map as it packed it: patched header)
        const uint8_t *p = mh.next;
        for (uint32_t i = 0; i < mh.len; i++) {
            const uint8_t *kend = mp_skip(p, m_end);
            const uint8_t *vend = kend ? mp_skip(kend, m_end) : nullptr;
            if (!vend) break;
            if (i != skip) {
                if (nappend > 0 || repack) { mp_canon(p, m_end, s); mp_canon(kend, m_end, s); }
                else s.copy(p, (uint32_t) (vend - p));
            }
            p = vend;
        }
    }
    else s.copy(m, (uint32_t) (m_end - m));
    if (nappend > 0) {
        const uint8_t *p = bm.next;
        for (uint32_t i = 0; i < bm.len; i++) {
            const uint8_t *kend = mp_skip(p, body_end);
            const uint8_t *vend = kend ? mp_skip(kend, body_end) : nullptr;
            if (!vend) break;
            bool take;
            if (cfg.reserve_data) take = !(plain_key && !cfg.preserve_key && null_test(cfg, caps.r, i, null_mask));
            else take = (i == ri.key_index);
            if (take) { mp_canon(p, kend, s); mp_canon(kend, vend, s); }
            p = vend;
        }
    }
    return true;
}
