// canon_walk.inc -- building a record again, for the lane-per-record filters that do (recmod, nest, typeconv, checklist, expect and
// kube _kernels.inc): the walk that sizes msgpack_pack_object's re-pack of an object and tells whether its bytes already are that
// re-pack, the bounded sink of the emit passes, the record's head, the body's map32 header, a span copy of any length and the walk
// over a body's entries that sends runs of already-canonical ones out as one span.  Every helper takes any sink it makes sense for
// (CountSink, ByteSink, BoundedSink).  Included inside namespace flbgpu after kdev.inc.

// one object at p (`open` containers around it): its end, nullptr when it is malformed, truncated or nested past the executor's limit.
// csize grows by the size of msgpack_pack_object's re-pack; canon is cleared when a header is not the one the packer writes.
DEV const uint8_t *canon_walk(const uint8_t *p, const uint8_t *end, uint32_t open, uint64_t &csize, bool &canon) {
    const uint8_t *p0 = p;
    uint64_t remaining = 1;
    uint32_t nopen = 0;
    while (remaining > 0) {
        Tok t = mp_tok(p, end);
        if (t.type == T_BAD) return nullptr;
        remaining--;
        const uint32_t c = ld8(p);
        const uint32_t raw = (uint32_t) (t.next - p);
        uint32_t pay = 0;
        CountSink h;
        switch (t.type) {
        case T_UINT: pk_uint(h, t.u); if (c >= 0xd0 && c <= 0xd3) canon = false; break;      // a signed header on a value >= 0
        case T_NINT: pk_int(h, (int64_t) t.u); break;
        case T_STR: pk_str_hdr(h, t.len); pay = t.len; break;
        case T_BIN: pk_bin_hdr(h, t.len); pay = t.len; break;
        case T_EXT: pk_ext_hdr(h, t.len, 0); pay = t.len; break;
        case T_ARRAY: pk_array_hdr(h, t.len); remaining += t.len; nopen++; break;
        case T_MAP: pk_map_hdr(h, t.len); remaining += 2ull * t.len; nopen++; break;
        default: h.n = raw; break;                                                          // nil, bool, float: one encoding
        }
        if ((uint32_t) h.n != raw) canon = false;
        csize += h.n + pay;
        p = t.next + pay;
    }
    if (open + nopen > MP_MAX_OPEN && !mp_depth_ok(p0, end, open)) return nullptr;
    return p;
}

// the body is a dynamic field of the reference's encoder: its map header is always map32 (flb_mp_map_header_init, src/flb_mp.c:591-603)
constexpr uint32_t MAP32_HDR = 5;


// the emit pass's sink: [p, limit) is the row's room.  Nothing is stored at or past limit; p keeps counting, so the caller sees
// both facts -- how long the record would have been and whether a store was withheld.
struct BoundedSink {
    uint8_t *p, *limit;
    bool over = false;
    DEV BoundedSink(uint8_t *dst, uint8_t *lim) : p(dst), limit(lim) {}
    DEV void note_exact() {}
    DEV void put(uint32_t b) {
        if (p < limit) *p = (uint8_t) b; else over = true;
        p++;
    }
    DEV void put32(uint32_t v) { for (int i = 0; i < 4; i++) put((v >> (8 * i)) & 0xffu); }
    DEV void copy(const uint8_t *src, uint32_t len) {
        const uint64_t room = p < limit ? (uint64_t) (limit - p) : 0;
        const uint32_t n = room < len ? (uint32_t) room : len;
        ByteSink bs(p);
        bs.copy(src, n);
        if (n < len) over = true;
        p += len;
    }
};

// a span of the record of any length
DEV void put_span(CountSink &s, const uint8_t *, uint64_t len) { s.n += len; }
template <class S> DEV void put_span(S &s, const uint8_t *src, uint64_t len) {
    while (len > 0x40000000ull) { s.copy(src, 0x40000000u); src += 0x40000000ull; len -= 0x40000000ull; }
    s.copy(src, (uint32_t) len);
}

// L bytes out of a table's words in LDS
template <class S> DEV void put_lds(S &s, const LDS_AS uint32_t *e, uint32_t L) {
    for (uint32_t j = 0; j < L; j++) s.put((e[j >> 2] >> (8 * (j & 3))) & 0xffu);
}

// a map32 header whose count is known later: its room is left open, and filled at the remembered address
DEV uint8_t *open_map32(CountSink &s) { s.n += MAP32_HDR; return nullptr; }
template <class S> DEV uint8_t *open_map32(S &s) { uint8_t *at = s.p; s.p += MAP32_HDR; return at; }
DEV void close_map32(CountSink &, uint8_t *, uint64_t) {}
DEV void close_map32(ByteSink &, uint8_t *at, uint64_t n) {
    ByteSink hs(at);
    hs.put(0xdf);
    hs.put32(__builtin_bswap32((uint32_t) n));
}
DEV void close_map32(BoundedSink &s, uint8_t *at, uint64_t n) {
    BoundedSink hs(at, s.limit);
    hs.put(0xdf);
    pk_be(hs, n, 4);
    if (hs.over) s.over = true;
}

// the record's head: [[EventTime(sec, nsec), -- fixarray 2, fixarray 2, fixext 8 of type 0
template <class S> DEV void put_event_head(S &s, uint32_t sec, uint32_t nsec) {
    s.put32(0x00d79292u);
    s.put32(__builtin_bswap32(sec));
    s.put32(__builtin_bswap32(nsec));
}
// the metadata re-packed; the empty map of an event in the legacy format
template <class S> DEV void put_meta(S &s, const Event &ev) {
    if (ev.meta) mp_canon(ev.meta, ev.meta_end, s); else s.put(0x80);
}

// the time of a record that goes out whatever flb_log_event_encoder_set_timestamp answers: the encoder refuses a time outside the
// EventTime range, the filter overwrites its answer and the record keeps the zero time begin_record left.  false: refused.
// NOT encoder_refuses_time (kdev.inc): that one lets the group markers' -1 s / -2 s pass, this one does not -- a difference no row
// shows today only because markers leave every filter before the time is looked at.
DEV bool event_time_or_zero(const Event &ev, uint32_t &sec, uint32_t &nsec) {
    const bool ok = ev.sec >= 0 && (uint64_t) ev.sec <= 0xffffffffull && ev.nsec >= 0 && ev.nsec < 1000000000LL;
    sec = ok ? (uint32_t) ev.sec : 0;
    nsec = ok ? (uint32_t) ev.nsec : 0;
    return ok;
}

// the entries of the body map bm into s, in order.  what(i, e0, v) says for entry i (key at e0, value at v): ENTRY_KEEP -- it goes
// out re-packed, and runs of kept entries whose bytes already are the packer's go out as one span; ENTRY_DROP -- nothing; ENTRY_OWN
// -- own(i, e0, v) writes it.  The open span is flushed before anything but a kept canonical entry is handled.  false: a key or a
// value is malformed, or the entries do not end at `end` (the row is one event and nothing else).
enum { ENTRY_KEEP, ENTRY_DROP, ENTRY_OWN };
struct EntryNoOwn { DEV void operator()(uint32_t, const uint8_t *, const uint8_t *) const {} };
template <class S, class W, class O = EntryNoOwn>
DEV bool put_entries(S &s, const Tok &bm, const uint8_t *end, W what, O own = O()) {
    const uint8_t *p = bm.next, *span = nullptr;
    for (uint32_t i = 0; i < bm.len; i++) {
        const uint8_t *e0 = p;
        uint64_t es = 0;
        bool canon = true;
        const uint8_t *v = canon_walk(p, end, 2, es, canon);
        if (!v) return false;
        p = canon_walk(v, end, 2, es, canon);
        if (!p) return false;
        const int w = what(i, e0, v);
        if (w == ENTRY_KEEP && canon) { if (!span) span = e0; continue; }
        if (span) { put_span(s, span, (uint64_t) (e0 - span)); span = nullptr; }
        if (w == ENTRY_KEEP) { mp_canon(e0, end, s, 2); mp_canon(v, end, s, 2); }
        else if (w == ENTRY_OWN) own(i, e0, v);
    }
    if (p != end) return false;
    if (span) put_span(s, span, (uint64_t) (p - span));
    return true;
}
