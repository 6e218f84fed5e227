// sp_select.inc -- sp_process_data (src/stream_processor/flb_sp.c:1607-1850) on the device: a SELECT without aggregation functions
// over one appended chunk.  Per record: WHERE (the same postfix program as the aggregate path, sp_kernels.inc sp_where), then
//   92 | the record's first element re-packed (msgpack_pack_object) | a map header in the width of the INCOMING map's size with the
//   number of entries written patched in afterwards (:1723,:1801-1815) | for every select key in order: `*` = every pair with a string
//   key; a name = one pair per entry of that name -- the key (or its alias), then flb_sp_key_to_value of the name: the FIRST entry's
//   value, sub-keys walked, nothing at all when that value is an array / bin / ext (the reference packs the key alone); NOW() /
//   UNIX_TIMESTAMP() / RECORD_TAG() = a pair packed once per call on the host, RECORD_TIME() = its key and the record's time as float64.
// A record none of whose keys exist leaves nothing (:1796-1799).  Two passes (size, emit) around a scan, one record per lane.

// the second half of flb_sp_key_to_value: first = the value of the first entry called like the key (nullptr: none)
DEV const uint8_t *sp_value_from_first(const SpPlan *pl, const SpKeyRef &k, const uint8_t *first, const uint8_t *end) {
    if (!first) return nullptr;
    const uint8_t *cur = first;

    Tok t = mp_tok(first, end);
    if (t.type == T_MAP && k.nsub > 0) {
        uint32_t matched = 0;
        bool found = false;
        for (uint32_t lv = 0; lv < k.nsub; lv++) {
            Tok cm = mp_tok(cur, end);
            if (cm.type != T_MAP) break;
            found = false;
            const uint8_t *q = cm.next;
            for (uint32_t i = 0; i < cm.len; i++) {
                Tok kk = mp_tok(q, end);
                const uint8_t *v = mp_skip(q, end, 3);
                if (!v) return nullptr;
                if (kk.type == T_STR && sp_name_eq(kk.next, kk.len, pl->blob + k.sub_off[lv], k.sub_len[lv])) { found = true; cur = v; matched++; break; }
                q = mp_skip(v, end, 3);
                if (!q) return nullptr;
            }
            if (matched == k.nsub) break;
        }
        if (!found || (matched > 0 && matched != k.nsub)) return nullptr;
    }
    const Tok vt = mp_tok(cur, end);
    if (vt.type == T_ARRAY || vt.type == T_BIN || vt.type == T_EXT || vt.type == T_BAD) return nullptr;    // msgpack_object_to_sp_value: -1
    return cur;
}


// flb_sp_key_to_value as a pointer to the value object (nullptr: NULL in the reference)
DEV const uint8_t *sp_value_ptr(const SpPlan *pl, const SpKeyRef &k, const uint8_t *map, const uint8_t *end) {
    Tok m = mp_tok(map, end);
    if (m.type != T_MAP) return nullptr;
    const uint8_t *p = m.next, *first = nullptr;
    for (uint32_t i = 0; i < m.len && !first; i++) {
        Tok kk = mp_tok(p, end);
        const uint8_t *v = mp_skip(p, end, 2);
        if (!v) return nullptr;
        if ((kk.type == T_STR || kk.type == T_BIN) && sp_name_eq(kk.next, kk.len, pl->blob + k.name_off, k.name_len)) first = v;     // (no type check: flb_sp_key.c:189)
        p = mp_skip(v, end, 2);
        if (!p) break;
    }
    return sp_value_from_first(pl, k, first, end);
}
// the selected pairs of one record; COUNT: only counts them
template <bool COUNT, class S> DEV uint32_t sp_select_pairs(const SpSelArgs &a, const SpHits &h, const uint8_t *map, const uint8_t *end, double ts, S &sk) {
    const SpPlan *pl = a.plan;
    const Tok m = mp_tok(map, end);
    uint32_t entries = 0;
    for (int si = 0; si < a.nsel; si++) {
        const SpSelKey &sel = a.sel[si];
        if (sel.star >= 2) {
            // flb_sp_func_time / flb_sp_func_record (:1732-1746): one entry whatever the record holds
            if (!COUNT) {
                for (uint32_t q = 0; q < sel.alias_len; q++) sk.put(ld8(a.consts + sel.alias_off + q));
                if (sel.star == 3) {
                    const uint64_t b = (uint64_t) __double_as_longlong(ts);
                    sk.put(0xcb);
                    for (int q = 7; q >= 0; q--) sk.put((uint8_t) (b >> (8 * q)));
                }
            }
            entries++;
            continue;
        }
        const SpKeyRef &kr = pl->keys[sel.key];
        if (!sel.star && h.fast) {
            // a named key: the record's one walk (sp_walk, made for WHERE) already knows its first value and how many string entries
            // carry the name -- a pair per entry, the key as the plan spells it (what msgpack_pack_object makes of the entry's own key)
            const uint8_t *f = h.first[0];
            uint32_t c = h.cnt[0];
            #pragma unroll
            for (int k = 1; k < SP_FAST_KEYS; k++) if (sel.key == (uint32_t) k) { f = h.first[k]; c = h.cnt[k]; }
            const uint32_t n = c;                                    // the string entries (sp_lookup)
            if (n && !COUNT) {
                const uint8_t *val = sp_value_from_first(pl, kr, f, end);
                for (uint32_t e = 0; e < n; e++) {
                    if (sel.has_alias) { pk_str_hdr(sk, sel.alias_len); for (uint32_t q = 0; q < sel.alias_len; q++) sk.put((uint8_t) pl->blob[sel.alias_off + q]); }
                    else { pk_str_hdr(sk, kr.name_len); for (uint32_t q = 0; q < kr.name_len; q++) sk.put((uint8_t) pl->blob[kr.name_off + q]); }
                    if (val) mp_canon(val, end, sk);
                }
            }
            entries += n;
            continue;
        }
        const uint8_t *val = nullptr;
        bool looked = false;
        const uint8_t *p = m.next;
        for (uint32_t i = 0; i < m.len; i++) {
            const Tok kk = mp_tok(p, end);
            const uint8_t *v = mp_skip(p, end, 2);
            const uint8_t *nx = v ? mp_skip(v, end, 2) : nullptr;
            if (!v || !nx) break;
            if (kk.type == T_STR) {
                if (sel.star) {
                    if (!COUNT) { mp_canon(p, end, sk); mp_canon(v, end, sk); }
                    entries++;
                }
                else if (sp_name_eq(kk.next, kk.len, pl->blob + kr.name_off, kr.name_len)) {
                    if (!COUNT) {
                        if (sel.has_alias) { pk_str_hdr(sk, sel.alias_len); for (uint32_t q = 0; q < sel.alias_len; q++) sk.put((uint8_t) pl->blob[sel.alias_off + q]); }
                        else mp_canon(p, end, sk);
                        if (!looked) { val = sp_value_ptr(pl, kr, map, end); looked = true; }
                        if (val) mp_canon(val, end, sk);
                    }
                    entries++;
                }
            }
            p = nx;
        }
    }
    return entries;
}

template <class S> DEV bool sp_select_record(const SpSelArgs &a, uint64_t r, const uint8_t *rec, const uint8_t *rec_end, S &sk, bool size_pass) {
    const SpPlan *pl = a.plan;
    SpHits h;
    h.fast = pl->nkeys <= SP_FAST_KEYS;
    Event ev = decode_event(rec, rec_end, h.fast);
    if (h.fast && (ev.flags & RF_VALID)) {
        const uint8_t *we = nullptr;
        if (!sp_walk(pl, ev.body, rec_end, h, &we) || we != rec_end) ev.flags = RF_BAD;
    }
    if (!(ev.flags & RF_VALID)) {
        if (size_pass) {
            if (mp_skip(rec, rec_end, 0) != rec_end) atomicMin(a.first_bad, (unsigned long long) r);
            else atomicOr(a.flags, (unsigned int) SPF_BAD_RECORD);
        }
        return false;
    }
    const uint8_t *map = ev.body, *end = ev.body_end;
    const double ts = (double) (uint64_t) (ev.sec < 0 ? 0x100000000ll + ev.sec : ev.sec) + (double) ev.nsec / 1000000000.0;
    bool defer = false;
    if (pl->nops != 0 && !sp_where<true>(pl, h, map, end, ts, a.flags, &defer)) return false;
    if (size_pass) atomicAdd(a.records, 1ull);
    CountSink none;
    const uint32_t entries = sp_select_pairs<true>(a, h, map, end, ts, none);
    if (entries == 0) return true;                                       // nothing of the record leaves
    const Tok m = mp_tok(map, end);
    sk.put(0x92);
    mp_canon(rec + 1, rec_end, sk);                                      // root.via.array.ptr[0]: [ts, metadata] (or the legacy timestamp)
    if (m.len <= 15) sk.put(0x80 | (entries & 0xFF));                    // (uint8_t) 0x8 << 4 | (uint8_t) map_entries
    else if (m.len <= 65535) { sk.put(0xde); sk.put((entries >> 8) & 255); sk.put(entries & 255); }
    else { sk.put(0xdf); sk.put(entries >> 24); sk.put((entries >> 16) & 255); sk.put((entries >> 8) & 255); sk.put(entries & 255); }
    sp_select_pairs<false>(a, h, map, end, ts, sk);
    return true;
}

template <bool EMIT>
__global__ void __launch_bounds__(256) k_sp_select(SpSelArgs a) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (uint64_t) gridDim.x * blockDim.x) {
        const uint8_t *rec = a.data + a.row_off[r], *rec_end = a.data + a.row_off[r + 1];
        if (!EMIT) {
            CountSink cs;
            a.out_len[r] = 0;
            if (rec != rec_end && sp_select_record(a, r, rec, rec_end, cs, true)) a.out_len[r] = (uint32_t) cs.n;
        }
        else if (a.out_off[r + 1] > a.out_off[r] && r < *a.first_bad) {
            ByteSink sk(a.out + a.out_off[r]);
            sp_select_record(a, r, rec, rec_end, sk, false);
        }
    }
}

void launch_sp_select(const SpSelArgs &a, bool emit, hipStream_t st) {
    if (a.n == 0) return;
    uint64_t b = (a.n + 255) / 256;
    if (b > 4096) b = 4096;
    if (emit) hipLaunchKernelGGL(k_sp_select<true>, dim3((unsigned) b), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_sp_select<false>, dim3((unsigned) b), dim3(256), 0, st, a);
}
