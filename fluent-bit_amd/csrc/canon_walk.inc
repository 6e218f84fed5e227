// canon_walk.inc -- what the lane-per-record filters that build records again share (recmod_kernels.inc, nest_kernels.inc): the walk
// that sizes msgpack_pack_object's re-pack of an object and tells whether its bytes already are that re-pack, the encoder's body
// header, and a span copy of any length.  Included inside namespace flbgpu after kdev.inc.

// one object at p (`open` containers around it): its end, nullptr when it is malformed, truncated or nested past the executor's limit.
// csize grows by the size of msgpack_pack_object's re-pack; canon is cleared when a header is not the one the packer writes.
DEV const uint8_t *rm_walk(const uint8_t *p, const uint8_t *end, uint32_t open, uint64_t &csize, bool &canon) {
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
constexpr uint32_t RM_MAP_HDR = 5;

DEV void rm_copy(ByteSink &bs, const uint8_t *src, uint64_t len) {
    while (len > 0x40000000ull) { bs.copy(src, 0x40000000u); src += 0x40000000ull; len -= 0x40000000ull; }
    bs.copy(src, (uint32_t) len);
}
