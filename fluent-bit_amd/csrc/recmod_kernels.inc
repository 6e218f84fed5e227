// recmod_kernels.inc -- filter_record_modifier (plugins/filter_record_modifier/filter_modifier.c:213-279, 298-486): a lane per
// record.  One walk over the body's top-level entries decides each key against the key table in LDS (make_bool_map) and adds up the
// canonical size of what stays; the body's order never changes and nothing is inserted between entries, so no entry list is kept.
// Two launches around the shared scan: the size pass writes every row's output length, the emit pass walks the body
// again, decides again (the table is in LDS, the key bytes are in the cache lines it copies anyway) and copies runs of adjacent kept
// entries whose encoding is already canonical as one span.  Included inside namespace flbgpu after kdev.inc,
// lane_rows.inc and canon_walk.inc.

struct RmTable {
    const LDS_AS uint32_t *w;       // the table's words in LDS
    int nkeys;
    int list;
};

// ASCII upper case -> lower case in the four bytes of a word (strncasecmp in the C locale; bytes >= 0x80 stay)
DEV uint32_t rm_fold4(uint32_t x) {
    const uint32_t h = x & 0x7f7f7f7fu;
    const uint32_t ge_a = h + 0x3f3f3f3fu;          // bit 7: low seven bits >= 'A'
    const uint32_t gt_z = h + 0x25252525u;          // bit 7: low seven bits >  'Z'
    const uint32_t m = ge_a & ~gt_z & ~x & 0x80808080u;
    return x | (m >> 2);
}
DEV uint32_t rm_fold1(uint32_t c) { return (c - 'A') < 26u ? c | 0x20u : c; }

// make_bool_map's inner loop (:248-270) for one STR / BIN key: does an entry of the table match?  An exact entry needs the same
// length, a prefix entry a key at least as long; then `length` bytes are compared without case -- never more than the key holds.
DEV bool rm_match(const RmTable &tb, const uint8_t *key, uint32_t klen) {
    for (int i = 0; i < tb.nkeys; i++) {
        const uint32_t lw = tb.w[2 * i];
        const uint32_t L = lw & ~RECMOD_PREFIX;
        if ((lw & RECMOD_PREFIX) ? klen < L : klen != L) continue;
        const LDS_AS uint32_t *e = tb.w + (tb.w[2 * i + 1] >> 2);
        uint32_t j = 0;
        bool eq = true;
        for (; eq && j + 4 <= L; j += 4) eq = rm_fold4(ldu32(key + j)) == e[j >> 2];
        if (eq && j < L) {
            const uint32_t last = e[j >> 2];
            for (uint32_t k = 0; eq && j + k < L; k++) eq = rm_fold1(ld8(key + j + k)) == ((last >> (8 * k)) & 0xffu);
        }
        if (eq) return true;
    }
    return false;
}

// is the entry with this key removed?  Only STR and BIN keys can match: with a remove list every other key stays, with an allow
// list it goes (:260-274)
DEV bool rm_removed(const RmTable &tb, const Tok &k) {
    if (tb.list == RECMOD_NONE) return false;
    const bool hit = (k.type == T_STR || k.type == T_BIN) && rm_match(tb, k.next, k.len);
    return hit == (tb.list == RECMOD_REMOVE);
}

struct RmRow {
    bool bad, decoded, wide, lost;      // decoder error / a record the callback saw / more than 65535 entries / a key was removed
    uint64_t len;                       // output bytes (0: nothing emitted)
};

// size pass: one record of cb_modifier_filter's loop (:351-463)
DEV RmRow rm_size(const RecmodArgs &a, const RmTable &tb, uint64_t r) {
    RmRow w;
    w.bad = false; w.decoded = false; w.wide = false; w.lost = false; w.len = 0;
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    if (rec == end) return w;                                         // a record an earlier filter dropped
    Event ev = decode_event(rec, end, true);
    if (ev.flags & RF_BAD) { w.bad = true; return w; }
    Tok bm = mp_tok(ev.body, end);
    uint64_t size = 0;
    uint32_t kept = 0;
    bool canon = true;
    const uint8_t *p = bm.next;
    for (uint32_t i = 0; i < bm.len; i++) {
        Tok k = mp_tok(p, end);
        uint64_t es = 0;
        p = canon_walk(p, end, 2, es, canon);
        if (p) p = canon_walk(p, end, 2, es, canon);
        if (!p) { w.bad = true; return w; }
        if (!rm_removed(tb, k)) { kept++; size += es; }
    }
    if (p != end) { w.bad = true; return w; }                         // the row is one event and nothing else
    if (ev.flags & RF_SKIP) return w;                                 // group markers: skipped by the decoder
    w.decoded = true;
    if (bm.len > 65535u) { w.wide = true; return w; }                 // BOOL_MAP_LIMIT (:369-377)
    w.lost = kept != bm.len;
    if (kept + a.nrec == 0) return w;                                 // (:408-410)
    CountSink cs;
    cs.n = 12 + MAP32_HDR;
    put_meta(cs, ev);
    w.len = cs.n + size + a.tail_len;
    return w;
}

// emit pass: the record whose length the size pass wrote
DEV void rm_emit(const RecmodArgs &a, const RmTable &tb, uint64_t r) {
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    Event ev = decode_event(rec, end, true);
    ByteSink bs(a.out + a.out_off[r]);
    uint32_t sec, nsec;
    event_time_or_zero(ev, sec, nsec);                                // (its answer is overwritten, :414-417)
    put_event_head(bs, sec, nsec);
    put_meta(bs, ev);
    uint8_t *hdr = open_map32(bs);                                    // the count is known when the walk is done
    // put_entries' walk without its checks (the size pass made them): with them this kernel measured 1 to 2 % slower (DESIGN 4n)
    Tok bm = mp_tok(ev.body, end);
    const uint8_t *p = bm.next, *span = nullptr;
    uint32_t kept = 0;
    for (uint32_t i = 0; i < bm.len; i++) {
        const uint8_t *e0 = p;
        Tok k = mp_tok(p, end);
        uint64_t es = 0;
        bool canon = true;
        const uint8_t *v = canon_walk(p, end, 2, es, canon);
        p = canon_walk(v, end, 2, es, canon);
        const bool keep = !rm_removed(tb, k);
        kept += keep ? 1u : 0u;
        if (keep && canon) { if (!span) span = e0; continue; }
        if (span) { put_span(bs, span, (uint64_t) (e0 - span)); span = nullptr; }
        if (keep) { mp_canon(e0, end, bs, 2); mp_canon(v, end, bs, 2); }
    }
    if (span) put_span(bs, span, (uint64_t) (p - span));
    if (a.tail_len) bs.copy(a.tail, a.tail_len);
    close_map32(bs, hdr, kept + a.nrec);
}

template <bool EMIT>
__global__ void __launch_bounds__(RECMOD_BLOCK) k_recmod(RecmodArgs a) {
    RmTable tb{lane_stage_table<RECMOD_BLOCK>(a.table, a.table_bytes), a.nkeys, a.list};
    __syncthreads();
    const uint64_t gsz = (uint64_t) gridDim.x * RECMOD_BLOCK;
    unsigned long long n_dec = 0, n_out = 0, n_lost = 0, n_big = 0;
    // lane_wave_rows' loop, written out: through the helper's lambda the emit pass measured 1 to 2 % slower on nest-shaped records
    // (DESIGN 4n).  Every wave walks in step (the trip count is the wave's, not the lane's): lane_count's ballots see whole waves.
    for (uint64_t r0 = (uint64_t) blockIdx.x * RECMOD_BLOCK + (threadIdx.x & ~63u); r0 < a.n; r0 += gsz) {
        const uint64_t r = r0 + (threadIdx.x & 63u);
        const bool live = r < a.n;
        if (EMIT) {
            if (live && a.len[r]) rm_emit(a, tb, r);
            continue;
        }
        RmRow w;
        w.bad = false; w.decoded = false; w.wide = false; w.lost = false; w.len = 0;
        if (live) {
            w = rm_size(a, tb, r);
            const bool big = w.len > 0xFFFFFFFFull;                    // a row the u32 length column cannot hold
            if (big) { n_big++; w.len = 0; }
            a.len[r] = (uint32_t) w.len;
            if (w.bad) atomicMin(a.first_bad, (unsigned long long) r);
            if (w.wide) atomicMin(a.first_wide, (unsigned long long) r);
        }
        lane_count(n_dec, w.decoded); lane_count(n_out, w.len != 0); lane_count(n_lost, w.lost);
    }
    if (EMIT) return;
    lane_flush(&a.counts[0], n_dec); lane_flush(&a.counts[1], n_out); lane_flush(&a.counts[2], n_lost);       // (lane 0's: one atomic a wave)
    lane_flush(&a.counts[3], n_big);
}

void launch_recmod(const RecmodArgs &a, bool emit, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 g(lane_blocks<RECMOD_BLOCK>(a.n)), b(RECMOD_BLOCK);
    if (emit) hipLaunchKernelGGL(k_recmod<true>, g, b, a.table_bytes, st, a);
    else hipLaunchKernelGGL(k_recmod<false>, g, b, a.table_bytes, st, a);
}
