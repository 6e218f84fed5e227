// tc_sink.inc -- the emit pass's bounded sink and what goes with it, shared by the lane-per-record filters that write a record through
// ONE function into a counting or a bounded sink (typeconv_kernels.inc, checklist_kernels.inc).  Included inside namespace flbgpu
// after kdev.inc and canon_walk.inc (RM_MAP_HDR).

// the emit pass's sink: [p, limit) is the row's room.  Nothing is stored at or past limit; p keeps counting, so the caller sees
// both facts -- how long the record would have been and whether a store was withheld.
struct TcSink {
    uint8_t *p, *limit;
    bool over = false;
    DEV TcSink(uint8_t *dst, uint8_t *lim) : p(dst), limit(lim) {}
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
DEV void tc_span(CountSink &s, const uint8_t *, uint64_t len) { s.n += len; }
DEV void tc_span(TcSink &s, const uint8_t *src, uint64_t len) {
    while (len > 0x40000000ull) { s.copy(src, 0x40000000u); src += 0x40000000ull; len -= 0x40000000ull; }
    s.copy(src, (uint32_t) len);
}
// the body's map32 header: its room is left open when the record begins and filled when the number of entries is known
DEV uint8_t *tc_open_hdr(CountSink &s) { s.n += RM_MAP_HDR; return nullptr; }
DEV uint8_t *tc_open_hdr(TcSink &s) { uint8_t *at = s.p; s.p += RM_MAP_HDR; return at; }
DEV void tc_close_hdr(CountSink &, uint8_t *, uint64_t) {}
DEV void tc_close_hdr(TcSink &s, uint8_t *at, uint64_t n) {
    TcSink hs(at, s.limit);
    hs.put(0xdf);
    pk_be(hs, n, 4);
    if (hs.over) s.over = true;
}

template <class S> DEV void tc_put_lds(S &s, const LDS_AS uint32_t *e, uint32_t L) {
    for (uint32_t j = 0; j < L; j++) s.put((e[j >> 2] >> (8 * (j & 3))) & 0xffu);
}
