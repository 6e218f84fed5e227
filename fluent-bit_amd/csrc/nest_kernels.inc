// nest_kernels.inc -- filter_nest (plugins/filter_nest/nest.c:298-345, 353-397, 473-606, 631-717): a lane per record.  One walk over
// the body's top-level entries decides each key against the table in LDS (the wildcards for nest, the key for lift) and adds up the
// canonical size of both halves of the output.  Two launches around the shared scan: the size pass writes every row's output length
// and whether the row goes out as its own bytes (no entry matched: emit_raw_record, :685-690) or is built again; the emit pass copies
// a raw row as one span and builds the others in two walks -- what stays, then what is nested or lifted.  Matching is strncmp on
// bytes (the table holds no NUL): a compare longer than the key takes the record's next bytes in, one that would need bytes past the
// record fails and is counted (the convention of mod_key_prefix).  Included inside namespace flbgpu after kdev.inc,
// lane_rows.inc and canon_walk.inc.

struct NestTable {
    const LDS_AS uint32_t *w;       // the table's words in LDS
    int op, nwild, pfx;
    bool has_key;
    uint32_t key_off, key_len, pfx_off, pfx_len;
};

// strncmp(key, entry, L) == 0 for an entry of L bytes at e: the bytes at `key` up to the record's end take part.  A compare that
// runs out of record before it finds a difference is counted in ovr and fails.
DEV bool nst_cmp(const LDS_AS uint32_t *e, uint32_t L, const uint8_t *key, const uint8_t *end, uint32_t &ovr) {
    const uint64_t room = (uint64_t) (end - key);
    const uint32_t avail = room < L ? (uint32_t) room : L;
    uint32_t j = 0;
    bool eq = true;
    for (; eq && j + 4 <= avail; j += 4) eq = ldu32(key + j) == e[j >> 2];
    for (; eq && j < avail; j++) eq = ld8(key + j) == ((e[j >> 2] >> (8 * (j & 3))) & 0xffu);
    if (!eq) return false;
    if (avail < L) { ovr++; return false; }
    return true;
}

// is_kv_to_nest (:298-345): STR and BIN keys only; an exact wildcard needs the same length, a prefix wildcard compares its own length
DEV bool nst_wild(const NestTable &tb, const Tok &k, const uint8_t *end, uint32_t &ovr) {
    if (k.type != T_STR && k.type != T_BIN) return false;
    for (int i = 0; i < tb.nwild; i++) {
        const uint32_t lw = tb.w[2 * i];
        const uint32_t L = lw & ~NEST_PREFIX;
        if (!(lw & NEST_PREFIX) && k.len != L) continue;
        if (nst_cmp(tb.w + (tb.w[2 * i + 1] >> 2), L, k.next, end, ovr)) return true;
    }
    return false;
}

// is_kv_to_lift (:353-397): a STR or BIN key equal to the key (a missing key has length 0) whose value is a map
DEV bool nst_lifted(const NestTable &tb, const Tok &k, const Tok &v, const uint8_t *end) {
    if ((k.type != T_STR && k.type != T_BIN) || k.len != tb.key_len || v.type != T_MAP) return false;
    uint32_t ovr = 0;                                                   // (the key's own bytes: inside the record)
    return nst_cmp(tb.w + (tb.key_off >> 2), tb.key_len, k.next, end, ovr);
}

// the key of a nested or lifted entry (map_transform_and_pack_each_fn :243-279, pack_map :421-453, the helpers :177-216): as it is
// without a prefix; with one always a STR, the prefix in front of it or cut off where the key starts with it.  undef: the reference
// reads a string out of a key that is neither STR nor BIN, or cuts a prefix off a key that is shorter than the prefix.
template <class S>
DEV void nst_key(const NestTable &tb, const Tok &k, const uint8_t *kp, const uint8_t *end, uint32_t open, S &s, uint32_t &ovr, bool &undef) {
    if (tb.pfx == NEST_PFX_NONE) { mp_canon(kp, end, s, open); return; }
    if (k.type != T_STR && k.type != T_BIN) { undef = true; return; }
    const LDS_AS uint32_t *pe = tb.w + (tb.pfx_off >> 2);
    if (tb.pfx == NEST_PFX_ADD) {
        pk_str_hdr(s, tb.pfx_len + k.len);
        put_lds(s, pe, tb.pfx_len);
        put_span(s, k.next, k.len);
        return;
    }
    uint32_t cut = 0;
    if (nst_cmp(pe, tb.pfx_len, k.next, end, ovr)) {
        if (k.len < tb.pfx_len) { undef = true; return; }
        cut = tb.pfx_len;
    }
    pk_str_hdr(s, k.len - cut);
    put_span(s, k.next + cut, k.len - cut);
}

struct NestRow {
    bool bad, decoded, built, undef;
    uint32_t mode, ovr;
    uint64_t len;                       // output bytes (0: nothing emitted)
};

// the entries of a lifted map at p (n of them), each key through nst_key, each value re-packed; nullptr: malformed
template <class S>
DEV const uint8_t *nst_inner(const NestTable &tb, const uint8_t *p, const uint8_t *end, uint32_t n, S &s, uint32_t &ovr, bool &undef) {
    for (uint32_t i = 0; i < n; i++) {
        Tok k = mp_tok(p, end);
        uint64_t cs = 0;
        bool canon = true;
        const uint8_t *v = canon_walk(p, end, 3, cs, canon);
        if (!v) return nullptr;
        nst_key(tb, k, p, end, 3, s, ovr, undef);
        p = mp_canon(v, end, s, 3);
        if (!p) return nullptr;
    }
    return p;
}

// size pass: one record of cb_nest_filter's loop (:671-691)
DEV NestRow nst_size(const NestArgs &a, const NestTable &tb, uint64_t r) {
    NestRow w;
    w.bad = false; w.decoded = false; w.built = false; w.undef = false; w.mode = NEST_ROW_NONE; w.ovr = 0; w.len = 0;
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    if (rec == end) return w;                                         // a record an earlier filter dropped
    Event ev = decode_event(rec, end, true);
    if (ev.flags & RF_BAD) { w.bad = true; return w; }
    // a record the rules would change is lost when the encoder refuses its time (set_timestamp, :506-511, :561-566) or, for nest,
    // the NULL key (:582-587): begin_record was called, nothing is committed and nothing goes out raw
    uint32_t sec, nsec;
    const bool lost = !event_time_or_zero(ev, sec, nsec) || (tb.op == NEST_OP_NEST && !tb.has_key);
    Tok bm = mp_tok(ev.body, end);
    CountSink moved;                                                  // the nested / lifted entries as they go out
    uint64_t stay = 0, nmatch = 0;
    uint32_t ovr = 0;
    bool undef = false;
    const uint8_t *p = bm.next;
    for (uint32_t i = 0; i < bm.len; i++) {
        Tok k = mp_tok(p, end);
        uint64_t ks = 0, vs = 0;
        bool canon = true;
        const uint8_t *v = canon_walk(p, end, 2, ks, canon);
        if (!v) { w.bad = true; return w; }
        if (tb.op == NEST_OP_NEST) {
            const uint8_t *q = canon_walk(v, end, 2, vs, canon);
            if (!q) { w.bad = true; return w; }
            if (nst_wild(tb, k, end, ovr)) {
                nmatch++;
                if (!lost) { nst_key(tb, k, p, end, 2, moved, ovr, undef); moved.n += vs; }
            }
            else stay += ks + vs;
            p = q;
        }
        else {
            Tok vt = mp_tok(v, end);
            if (nst_lifted(tb, k, vt, end)) {
                nmatch++;
                p = lost ? mp_skip(v, end, 2) : nst_inner(tb, vt.next, end, vt.len, moved, ovr, undef);
                if (!p) { w.bad = true; return w; }
            }
            else {
                p = canon_walk(v, end, 2, vs, canon);
                if (!p) { w.bad = true; return w; }
                stay += ks + vs;
            }
        }
    }
    if (p != end) { w.bad = true; return w; }                         // the row is one event and nothing else
    if (ev.flags & RF_SKIP) return w;                                 // group markers: skipped by the decoder
    w.decoded = true;
    w.ovr = ovr;
    if (nmatch == 0) { w.mode = NEST_ROW_RAW; w.len = (uint64_t) (end - rec); return w; }
    if (lost) return w;
    if (undef) { w.undef = true; w.mode = NEST_ROW_RAW; w.len = (uint64_t) (end - rec); return w; }
    CountSink cs;
    cs.n = 12 + MAP32_HDR;
    put_meta(cs, ev);
    if (tb.op == NEST_OP_NEST) { pk_str_hdr(cs, tb.key_len); cs.n += tb.key_len + MAP32_HDR; }
    w.built = true;
    w.mode = NEST_ROW_BUILT;
    w.len = cs.n + stay + moved.n;
    return w;
}

// emit pass: a row the size pass marked as built again
DEV void nst_emit(const NestArgs &a, const NestTable &tb, uint64_t r) {
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    Event ev = decode_event(rec, end, true);
    ByteSink bs(a.out + a.out_off[r]);
    put_event_head(bs, (uint32_t) ev.sec, (uint32_t) ev.nsec);
    put_meta(bs, ev);
    uint8_t *hdr = open_map32(bs);                                    // the count is known when the walk is done
    Tok bm = mp_tok(ev.body, end);
    uint32_t ovr = 0;
    bool undef = false;
    // what stays, in order: runs of entries whose encoding is already canonical go out as one span.  put_entries' walk without its
    // checks (the size pass made them): with them nst_emit measured about 1 % slower on lifted maps (DESIGN 4n)
    const uint8_t *p = bm.next, *span = nullptr;
    uint64_t kept = 0, nmatch = 0;
    for (uint32_t i = 0; i < bm.len; i++) {
        const uint8_t *e0 = p;
        Tok k = mp_tok(p, end);
        uint64_t es = 0;
        bool canon = true;
        const uint8_t *v = canon_walk(p, end, 2, es, canon);
        p = canon_walk(v, end, 2, es, canon);
        const bool hit = tb.op == NEST_OP_NEST ? nst_wild(tb, k, end, ovr) : nst_lifted(tb, k, mp_tok(v, end), end);
        nmatch += hit ? 1u : 0u;
        kept += hit ? 0u : 1u;
        if (!hit && canon) { if (!span) span = e0; continue; }
        if (span) { put_span(bs, span, (uint64_t) (e0 - span)); span = nullptr; }
        if (!hit) { mp_canon(e0, end, bs, 2); mp_canon(v, end, bs, 2); }
    }
    if (span) put_span(bs, span, (uint64_t) (p - span));
    uint64_t lifted = 0;
    if (tb.op == NEST_OP_NEST) {
        // the key as a STR and the nested map; the encoder's scopes always write map32 (src/flb_mp.c:591-603)
        pk_str_hdr(bs, tb.key_len);
        put_lds(bs, tb.w + (tb.key_off >> 2), tb.key_len);
        close_map32(bs, open_map32(bs), nmatch);
    }
    p = bm.next;
    for (uint32_t i = 0; i < bm.len && nmatch > 0; i++) {
        Tok k = mp_tok(p, end);
        const uint8_t *k0 = p;
        const uint8_t *v = mp_skip(p, end, 2);
        if (tb.op == NEST_OP_NEST) {
            if (nst_wild(tb, k, end, ovr)) {
                nmatch--;
                nst_key(tb, k, k0, end, 2, bs, ovr, undef);
                p = mp_canon(v, end, bs, 2);
            }
            else p = mp_skip(v, end, 2);
        }
        else {
            Tok vt = mp_tok(v, end);
            if (nst_lifted(tb, k, vt, end)) {
                nmatch--;
                lifted += vt.len;
                p = nst_inner(tb, vt.next, end, vt.len, bs, ovr, undef);
            }
            else p = mp_skip(v, end, 2);
        }
    }
    close_map32(bs, hdr, kept + (tb.op == NEST_OP_NEST ? 1u : lifted));
}

template <bool EMIT>
__global__ void __launch_bounds__(NEST_BLOCK) k_nest(NestArgs a) {
    NestTable tb{lane_stage_table<NEST_BLOCK>(a.table, a.table_bytes), a.op, a.nwild, a.pfx, a.has_key != 0, a.key_off, a.key_len, a.pfx_off, a.pfx_len};
    __syncthreads();
    unsigned long long n_dec = 0, n_out = 0, n_built = 0, n_undef = 0, n_big = 0, n_ovr = 0;
    lane_wave_rows<NEST_BLOCK>(a.n, [&](uint64_t r, bool live) {
        if (EMIT) {
            if (live && a.len[r]) {
                if (a.mode[r] == NEST_ROW_BUILT) nst_emit(a, tb, r);
                else {
                    ByteSink bs(a.out + a.out_off[r]);
                    put_span(bs, a.data + a.row_off[r], a.row_off[r + 1] - a.row_off[r]);
                }
            }
            return;
        }
        NestRow w;
        w.bad = false; w.decoded = false; w.built = false; w.undef = false; w.mode = NEST_ROW_NONE; w.ovr = 0; w.len = 0;
        if (live) {
            w = nst_size(a, tb, r);
            const bool big = w.len > 0xFFFFFFFFull;                    // a row the u32 length column cannot hold
            if (big) { n_big++; w.len = 0; w.built = false; w.mode = NEST_ROW_NONE; }
            a.len[r] = (uint32_t) w.len;
            a.mode[r] = (uint8_t) w.mode;
            n_ovr += w.ovr;
            if (w.bad) atomicMin(a.first_bad, (unsigned long long) r);
        }
        lane_count(n_dec, w.decoded); lane_count(n_out, w.len != 0); lane_count(n_built, w.built); lane_count(n_undef, w.undef);
    });
    if (EMIT) return;
    lane_flush(&a.counts[0], n_dec); lane_flush(&a.counts[1], n_out); lane_flush(&a.counts[2], n_built);      // (lane 0's: one atomic a wave)
    lane_flush(&a.counts[5], n_undef);
    lane_flush(&a.counts[3], n_big); lane_flush(&a.counts[4], n_ovr);
}

void launch_nest(const NestArgs &a, bool emit, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 g(lane_blocks<NEST_BLOCK>(a.n)), b(NEST_BLOCK);
    if (emit) hipLaunchKernelGGL(k_nest<true>, g, b, a.table_bytes, st, a);
    else hipLaunchKernelGGL(k_nest<false>, g, b, a.table_bytes, st, a);
}
