// modify_kernels.inc -- filter_modify (plugins/filter_modify/modify.c:523-1457): a lane per record.  The lane decodes the event,
// lists the body's entries once, evaluates the conditions on that original list, then runs the rule program as edits of the list
// (entries keep pointing at their original key and value, or at a string a rule wrote) -- the map is never re-packed per rule.
// String and regex tests give the same answers on the original bytes as on msgpack_pack_object's re-pack: re-packing changes
// headers, never STR / BIN payloads.  The one place where the re-packed bytes themselves matter is the prefix test's overread
// (mod_key_prefix).  Two launches and a scan: the size pass writes every row's output length, the emit pass writes the rows.
// Included inside namespace flbgpu after kdev.inc and lane_rows.inc.

DEV uint32_t me_koff(uint64_t e) { return (uint32_t) e; }
DEV uint32_t me_kid(uint64_t e) { return (uint32_t) (e >> 32) & 0xFFu; }
DEV uint32_t me_vid(uint64_t e) { return (uint32_t) (e >> 40) & 0xFFu; }
DEV bool me_marked(uint64_t e) { return (e >> 48) & 1u; }
DEV uint64_t me_make(uint32_t koff, uint32_t kid, uint32_t vid) { return (uint64_t) koff | ((uint64_t) kid << 32) | ((uint64_t) vid << 40); }
constexpr uint32_t ME_NONE = 0xFFu;
constexpr uint64_t ME_MARK = 1ull << 48;

// the entry list of one lane: in LDS entry i of every lane of the workgroup sits side by side (stride MOD_BLOCK: the lanes of a wave
// that walk their lists in step touch 64 consecutive u64, no bank is hit twice), in the HBM arena the entries are contiguous (stride 1)
struct MTab {
    uint64_t *p;                  // (a generic pointer: LDS or HBM)
    uint32_t stride;
    DEV uint64_t &operator[](uint32_t i) const { return p[(uint64_t) i * stride]; }
};

struct MRow {
    const uint8_t *rec, *end;
    MTab tab;
    uint32_t cnt;
    bool repacked;                // a rule has applied: the current buffer is the canonical re-pack of the map
    bool overread;                // a prefix test ran past the bytes the reference would have read inside the record
};

DEV bool mem_eq(const uint8_t *a, const uint8_t *b, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) if (ld8(a + i) != ld8(b + i)) return false;
    return true;
}
DEV void mod_str(const ModArgs &a, uint32_t id, const uint8_t *&s, uint32_t &len) {
    const ModRule &r = a.rules[id >> 1];
    if (id & 1) { s = a.str + r.v_off; len = r.v_len; }
    else { s = a.str + r.k_off; len = r.k_len; }
}
DEV const uint8_t *me_val(const MRow &w, uint64_t e) { return mp_skip(w.rec + me_koff(e), w.end, 2); }

// helper_msgpack_object_matches_regex (:523-552): STR as it is, BOOLEAN as the text true / false, everything else never matches
DEV bool mod_rx_text(const GrepRule &ru, const uint8_t *s, uint32_t len) {
    int m = dfa_match(ru.dfa.cls, ru.dfa.ddelta, ru.dfa.d_final, ru.dfa.ncls, ru.dfa.d_init, s, len);
    if (m == RX_POISON) m = rx_match_handed_on(ru.utf8, s, len) ? RX_MATCH : RX_NOMATCH;
    return m == RX_MATCH;
}
DEV bool mod_rx_obj(const ModArgs &a, const GrepRule &ru, const uint8_t *p, const uint8_t *end) {
    Tok t = mp_tok(p, end);
    if (t.type == T_BOOL) return t.u ? mod_rx_text(ru, a.str + a.true_off, 4) : mod_rx_text(ru, a.str + a.false_off, 5);
    if (t.type != T_STR) return false;
    return mod_rx_text(ru, t.next, t.len);
}
DEV bool mod_key_rx(const ModArgs &a, const MRow &w, uint64_t e, const GrepRule &ru) {
    const uint32_t kid = me_kid(e);
    if (kid != ME_NONE) { const uint8_t *s; uint32_t l; mod_str(a, kid, s, l); return mod_rx_text(ru, s, l); }
    return mod_rx_obj(a, ru, w.rec + me_koff(e), w.end);
}
DEV bool mod_val_rx(const ModArgs &a, const MRow &w, uint64_t e, const GrepRule &ru) {
    const uint32_t vid = me_vid(e);
    if (vid != ME_NONE) { const uint8_t *s; uint32_t l; mod_str(a, vid, s, l); return mod_rx_text(ru, s, l); }
    return mod_rx_obj(a, ru, me_val(w, e), w.end);
}
// helper_msgpack_object_matches_str (:656-677): STR or BIN of the same length and bytes
DEV bool mod_key_eq(const ModArgs &a, const MRow &w, uint64_t e, const uint8_t *s, uint32_t len) {
    const uint32_t kid = me_kid(e);
    if (kid != ME_NONE) { const uint8_t *q; uint32_t l; mod_str(a, kid, q, l); return l == len && mem_eq(q, s, len); }
    Tok t = mp_tok(w.rec + me_koff(e), w.end);
    return (t.type == T_STR || t.type == T_BIN) && t.len == len && mem_eq(t.next, s, len);
}

// compares what is put into it with `left` bytes of a rule string
struct CmpSink {
    const uint8_t *s;
    uint32_t left;
    bool done = false, eq = false;
    DEV void put(uint32_t b) {
        if (done) return;
        if ((uint8_t) b != ld8(s)) { done = true; return; }
        s++;
        if (--left == 0) { done = true; eq = true; }
    }
    DEV void copy(const uint8_t *src, uint32_t len) { for (uint32_t i = 0; i < len && !done; i++) put(ld8(src + i)); }
    DEV void note_exact() {}
};

// msgpack_pack_object of an entry's key / value, a written string as STR
template <class S> DEV void mod_canon_key(const ModArgs &a, const MRow &w, uint64_t e, S &s) {
    const uint32_t kid = me_kid(e);
    if (kid != ME_NONE) { const uint8_t *q; uint32_t l; mod_str(a, kid, q, l); pk_str_hdr(s, l); s.copy(q, l); }
    else mp_canon(w.rec + me_koff(e), w.end, s, 2);
}
template <class S> DEV void mod_canon_val(const ModArgs &a, const MRow &w, uint64_t e, S &s) {
    const uint32_t vid = me_vid(e);
    if (vid != ME_NONE) { const uint8_t *q; uint32_t l; mod_str(a, vid, q, l); pk_str_hdr(s, l); s.copy(q, l); }
    else mp_canon(me_val(w, e), w.end, s, 2);
}

// helper_msgpack_object_matches_wildcard (:599-616): strncmp(rule, key, rule_len) on STR or BIN keys.  A key shorter than the rule
// lets the bytes behind it in the CURRENT buffer take part: the record itself before the first rule that applied, the canonical
// re-pack of the map after it.  A compare that would need bytes past the record (or past the re-packed map) is counted and fails.
DEV bool mod_key_prefix(const ModArgs &a, MRow &w, uint32_t j, const uint8_t *s, uint32_t L) {
    const uint64_t e = w.tab[j];
    const uint8_t *kp;
    uint32_t kl;
    const uint32_t kid = me_kid(e);
    if (kid != ME_NONE) mod_str(a, kid, kp, kl);
    else {
        Tok t = mp_tok(w.rec + me_koff(e), w.end);
        if (t.type != T_STR && t.type != T_BIN) return false;
        kp = t.next; kl = t.len;
    }
    const uint32_t m = kl < L ? kl : L;
    if (!mem_eq(kp, s, m)) return false;
    if (kl >= L) return true;
    if (!w.repacked) {
        const uint8_t *p = kp + kl;
        for (uint32_t i = 0; i < L - kl; i++) {
            if (p + i >= w.end) { w.overread = true; return false; }
            if (ld8(p + i) != ld8(s + kl + i)) return false;
        }
        return true;
    }
    CmpSink cs{s + kl, L - kl};
    mod_canon_val(a, w, e, cs);
    for (uint32_t k = j + 1; k < w.cnt && !cs.done; k++) {
        mod_canon_key(a, w, w.tab[k], cs);
        if (!cs.done) mod_canon_val(a, w, w.tab[k], cs);
    }
    if (cs.done) return cs.eq;
    w.overread = true;
    return false;
}

// flb_ra_get_kv_pair (src/flb_record_accessor.c:790-800, src/flb_ra_key.c:108-135,151-336) on the original body: the LAST entry
// whose key is a STR equal to the name, then the sub-keys; *val = the value.  A path that ends on an array index has no key object
// and every condition reads that as "not found" (modify.c:754-757).
DEV bool mod_lookup(const ModArgs &a, const MRow &w, const DevKey &k, const uint8_t **val) {
    const uint8_t *v = nullptr;
    for (uint32_t i = 0; i < w.cnt; i++) {
        const uint64_t e = w.tab[i];
        Tok t = mp_tok(w.rec + me_koff(e), w.end);
        if (t.type == T_STR && t.len == (uint32_t) k.key_len && mem_eq(t.next, (const uint8_t *) k.key, t.len)) v = me_val(w, e);
    }
    if (!v) return false;
    Tok vt = mp_tok(v, w.end);
    if ((vt.type == T_MAP || vt.type == T_ARRAY) && k.nsub > 0) {
        const uint8_t *d = ra_descend(k, v, w.end);
        if (!d || k.sub_is_index[k.nsub - 1]) return false;
        v = d;
    }
    *val = v;
    return true;
}

DEV bool mod_cond(const ModArgs &a, const MRow &w, const ModCond &c) {
    switch (c.type) {
    case MC_A_KEY_MATCHES: case MC_NO_KEY_MATCHES: {
        bool any = false;
        for (uint32_t i = 0; i < w.cnt && !any; i++) any = mod_key_rx(a, w, w.tab[i], a.rx[c.rx_a]);
        return c.type == MC_A_KEY_MATCHES ? any : !any;
    }
    case MC_MATCHING_KEYS_HAVE_MATCHING_VALUES: case MC_MATCHING_KEYS_DO_NOT_HAVE_MATCHING_VALUES: {
        bool all = true;
        for (uint32_t i = 0; i < w.cnt && all; i++)
            if (mod_key_rx(a, w, w.tab[i], a.rx[c.rx_a]) && !mod_val_rx(a, w, w.tab[i], a.rx[c.rx_b])) all = false;
        return c.type == MC_MATCHING_KEYS_HAVE_MATCHING_VALUES ? all : !all;
    }
    default: break;
    }
    const uint8_t *v = nullptr;
    const bool found = c.key >= 0 && mod_lookup(a, w, a.keys[c.key], &v);
    switch (c.type) {
    case MC_KEY_EXISTS: return found;
    case MC_KEY_DOES_NOT_EXIST: return !found;
    case MC_KEY_VALUE_EQUALS: case MC_KEY_VALUE_DOES_NOT_EQUAL: {
        if (!found) return false;
        Tok t = mp_tok(v, w.end);
        const bool eq = (t.type == T_STR || t.type == T_BIN) && t.len == c.b_len && mem_eq(t.next, a.str + c.b_off, t.len);
        return c.type == MC_KEY_VALUE_EQUALS ? eq : !eq;
    }
    case MC_KEY_VALUE_MATCHES: case MC_KEY_VALUE_DOES_NOT_MATCH: {
        if (!found) return false;
        const bool m = mod_rx_obj(a, a.rx[c.rx_b], v, w.end);
        return c.type == MC_KEY_VALUE_MATCHES ? m : !m;
    }
    default: return false;
    }
}

// the entries a rule's key names (marked); returns how many
DEV uint32_t mod_mark(const ModArgs &a, MRow &w, const ModRule &r) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < w.cnt; i++) {
        bool m;
        if (r.type == MR_REMOVE_REGEX) m = mod_key_rx(a, w, w.tab[i], a.rx[r.rx]);
        else if (r.type == MR_REMOVE_WILDCARD || r.type == MR_MOVE_TO_START || r.type == MR_MOVE_TO_END) m = mod_key_prefix(a, w, i, a.str + r.k_off, r.k_len);
        else m = mod_key_eq(a, w, w.tab[i], a.str + r.k_off, r.k_len);
        if (m) { w.tab[i] |= ME_MARK; n++; }
    }
    return n;
}
DEV uint32_t mod_count_val(const ModArgs &a, const MRow &w, const ModRule &r) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < w.cnt; i++) n += mod_key_eq(a, w, w.tab[i], a.str + r.v_off, r.v_len) ? 1u : 0u;
    return n;
}
DEV void mod_unmark(MRow &w) { for (uint32_t i = 0; i < w.cnt; i++) w.tab[i] &= ~ME_MARK; }
DEV void mod_drop_marked(MRow &w) {
    uint32_t o = 0;
    for (uint32_t i = 0; i < w.cnt; i++) if (!me_marked(w.tab[i])) w.tab[o++] = w.tab[i];
    w.cnt = o;
}
// stable partition: the marked entries first (to_start) or last
DEV void mod_partition(MRow &w, bool to_start) {
    uint32_t o = 0;
    for (uint32_t i = 0; i < w.cnt; i++) {
        if (me_marked(w.tab[i]) == to_start) {
            const uint64_t e = w.tab[i];
            for (uint32_t k = i; k > o; k--) w.tab[k] = w.tab[k - 1];
            w.tab[o++] = e;
        }
    }
    mod_unmark(w);
}
DEV void mod_insert(MRow &w, uint32_t at, uint64_t e) {
    for (uint32_t k = w.cnt; k > at; k--) w.tab[k] = w.tab[k - 1];
    w.tab[at] = e;
    w.cnt++;
}
DEV uint64_t mod_renamed(uint64_t e, uint32_t id) { return me_make(me_koff(e), id, me_vid(e)); }

// apply_modifying_rule (:955-1337); true when the rule applied
DEV bool mod_rule(const ModArgs &a, MRow &w, int ri) {
    const ModRule &r = a.rules[ri];
    const uint32_t kid = 2u * (uint32_t) ri, vid = kid + 1;
    const uint32_t mk = mod_mark(a, w, r);
    switch (r.type) {
    case MR_RENAME: {
        if (mk == 0 || mod_count_val(a, w, r) > 0) { mod_unmark(w); return false; }
        for (uint32_t i = 0; i < w.cnt; i++) if (me_marked(w.tab[i])) w.tab[i] = mod_renamed(w.tab[i], vid);
        return true;
    }
    case MR_HARD_RENAME: {
        if (mk == 0) return false;
        const uint32_t cf = mod_count_val(a, w, r);
        uint32_t o = 0;
        for (uint32_t i = 0; i < w.cnt; i++) {
            const uint64_t e = w.tab[i];
            if (cf > 0 && mod_key_eq(a, w, e, a.str + r.v_off, r.v_len)) continue;
            w.tab[o++] = me_marked(e) ? mod_renamed(e, vid) : e;
        }
        w.cnt = o;
        return true;
    }
    case MR_COPY: case MR_HARD_COPY: {
        if (mk != 1) { mod_unmark(w); return false; }
        const uint32_t cf = mod_count_val(a, w, r);
        if ((r.type == MR_COPY && cf > 0) || cf > 1) { mod_unmark(w); return false; }
        if (cf == 1) {             // Hard_copy: the target goes, the copy takes its place behind the source
            uint32_t o = 0;
            for (uint32_t i = 0; i < w.cnt; i++) if (!mod_key_eq(a, w, w.tab[i], a.str + r.v_off, r.v_len)) w.tab[o++] = w.tab[i];
            w.cnt = o;
        }
        for (uint32_t i = 0; i < w.cnt; i++) {
            if (me_marked(w.tab[i])) {
                w.tab[i] &= ~ME_MARK;
                mod_insert(w, i + 1, mod_renamed(w.tab[i], vid));
                break;
            }
        }
        return true;
    }
    case MR_ADD:
        if (mk > 0) { mod_unmark(w); return false; }
        w.tab[w.cnt++] = me_make(0xFFFFFFFFu, kid, vid);
        return true;
    case MR_SET:
        mod_drop_marked(w);
        w.tab[w.cnt++] = me_make(0xFFFFFFFFu, kid, vid);
        return true;
    case MR_REMOVE: case MR_REMOVE_WILDCARD: case MR_REMOVE_REGEX:
        if (mk == 0) return false;
        mod_drop_marked(w);
        return true;
    case MR_MOVE_TO_START: case MR_MOVE_TO_END:
        if (mk == 0) return false;
        mod_partition(w, r.type == MR_MOVE_TO_START);
        return true;
    default:
        mod_unmark(w);
        return false;
    }
}

// one record: 0 = not decoded (marker, dropped row, decoder error: *bad), else the output length; *rebuilt = the record is re-encoded
template <bool EMIT>
DEV uint64_t mod_record(const ModArgs &a, uint64_t r, uint64_t *lds_tab, bool *bad, bool *decoded, bool *rebuilt, bool *over) {
    *bad = false; *decoded = false; *rebuilt = false; *over = false;
    MRow w;
    w.rec = a.data + a.row_off[r]; w.end = a.data + a.row_off[r + 1];
    w.repacked = false; w.overread = false;
    if (w.rec == w.end) return 0;                                     // a record an earlier filter dropped
    Event ev = decode_event(w.rec, w.end);
    if ((ev.flags & RF_BAD) || ev.body_end != w.end) { *bad = true; return 0; }
    if (ev.flags & RF_SKIP) return 0;                                 // group markers: skipped by the decoder
    *decoded = true;
    Tok bm = mp_tok(ev.body, w.end);
    const uint64_t need = (uint64_t) bm.len + (uint64_t) a.grow;
    if (need <= (uint64_t) MOD_LDS_ENTRIES) w.tab = MTab{lds_tab, (uint32_t) MOD_BLOCK};
    else {
        const unsigned long long base = atomicAdd(a.arena_top, (unsigned long long) need);
        if (!EMIT) atomicAdd(&a.counts[3], (unsigned long long) need);
        if (base + need > a.arena_cap) { *over = true; return 0; }   // the host grows the arena and runs the call again
        w.tab = MTab{a.arena + base, 1u};
    }
    const uint8_t *p = bm.next;
    for (uint32_t i = 0; i < bm.len; i++) {
        w.tab[i] = me_make((uint32_t) (p - w.rec), ME_NONE, ME_NONE);
        p = mp_skip(p, w.end, 2);
        p = mp_skip(p, w.end, 2);
    }
    w.cnt = bm.len;
    bool ok = true;
    for (int c = 0; c < a.nconds; c++) if (!mod_cond(a, w, a.conds[c])) ok = false;
    bool applied = false;
    if (ok) for (int i = 0; i < a.nrules; i++) if (mod_rule(a, w, i)) { applied = true; w.repacked = true; }
    if (!EMIT && w.overread) atomicAdd(&a.counts[2], 1ull);
    const uint64_t raw = (uint64_t) (w.end - w.rec);
    // the encoder refuses a time outside the EventTime range: the record is rolled back and copied as it came (:1442-1448)
    if (!applied || ev.sec < 0 || (uint64_t) ev.sec > 0xffffffffull || ev.nsec < 0 || ev.nsec >= 1000000000LL) {
        if (EMIT) { ByteSink bs(a.out + a.out_off[r]); bs.copy(w.rec, (uint32_t) raw); }
        return raw;
    }
    *rebuilt = true;
    if (EMIT) {
        ByteSink bs(a.out + a.out_off[r]);
        bs.put(0x92); bs.put(0x92); bs.put(0xd7); bs.put(0x00);
        pk_be(bs, (uint64_t) ev.sec, 4); pk_be(bs, (uint64_t) ev.nsec, 4);
        if (ev.meta) mp_canon(ev.meta, ev.meta_end, bs); else bs.put(0x80);
        pk_map_hdr(bs, w.cnt);
        for (uint32_t i = 0; i < w.cnt; i++) { mod_canon_key(a, w, w.tab[i], bs); mod_canon_val(a, w, w.tab[i], bs); }
        return (uint64_t) (bs.p - (a.out + a.out_off[r]));
    }
    CountSink cs;
    cs.n = 12;
    if (ev.meta) mp_canon(ev.meta, ev.meta_end, cs); else cs.n += 1;
    pk_map_hdr(cs, w.cnt);
    for (uint32_t i = 0; i < w.cnt; i++) { mod_canon_key(a, w, w.tab[i], cs); mod_canon_val(a, w, w.tab[i], cs); }
    return cs.n;
}

template <bool EMIT>
__global__ void __launch_bounds__(MOD_BLOCK) k_modify(ModArgs a) {
    __shared__ uint64_t s_tab[MOD_BLOCK * MOD_LDS_ENTRIES];
    uint64_t *tab = s_tab + threadIdx.x;                             // entry i at s_tab[i * MOD_BLOCK + lane]
    const uint64_t gsz = (uint64_t) gridDim.x * blockDim.x;
    unsigned long long n_dec = 0, n_mod = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += gsz) {
        bool bad, decoded, rebuilt, over;
        const uint64_t len = mod_record<EMIT>(a, r, tab, &bad, &decoded, &rebuilt, &over);
        if (EMIT) continue;
        if (bad) atomicMin(a.first_bad, (unsigned long long) r);
        if (over) atomicAdd(&a.counts[4], 1ull);
        if (len > 0xFFFFFFFFull) atomicAdd(&a.counts[4], 1ull << 32);  // a row the u32 length column cannot hold
        a.len[r] = (uint32_t) len;
        n_dec += decoded ? 1 : 0;
        n_mod += rebuilt ? 1 : 0;
    }
    if (!EMIT) {
        if (n_dec) atomicAdd(&a.counts[0], n_dec);
        if (n_mod) atomicAdd(&a.counts[1], n_mod);
    }
}

void launch_modify(const ModArgs &a, bool emit, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 g(lane_blocks<MOD_BLOCK>(a.n)), b(MOD_BLOCK);
    if (emit) hipLaunchKernelGGL(k_modify<true>, g, b, 0, st, a);
    else hipLaunchKernelGGL(k_modify<false>, g, b, 0, st, a);
}
