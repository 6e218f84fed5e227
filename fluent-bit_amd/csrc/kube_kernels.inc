// kube_kernels.inc -- filter_kubernetes' per-record half (plugins/filter_kubernetes/kubernetes.c:112-137 get_stream, 139-161
// value_trim_size, 163-247 merge_log_handler, 318-644 pack_map_content, 733-850 the record loop): a lane per record, the configuration
// and merge_log_key in LDS.  k_kube<KB_SIZE> decodes the row, decides its stream and whether the pod's properties exclude it, finds
// `log`, runs flb_pack_json_recs' rules on it (json_dev.inc's value walker, as pjson_dev.inc does) and sizes the rebuilt record into a
// counting sink; k_kube<KB_EMIT> writes every row into its own [out_off[r], out_off[r + 1]) through the bounded sink and no further.
// ONE function, kb_record, writes a record into either sink, so both passes walk the same code.
//
// What every record ends on -- "kubernetes" + the pod map, "kubernetes_namespace" + the namespace map: the tail, usually more bytes
// than the record in front of it -- is not written by the lanes: when the lanes of a wave have written their own part, the wave copies
// the tail behind each of its records with all 64 lanes (kb_append), out of LDS when the tail fits the budget, else out of HBM / L2.
// The EXACT instantiation (wide bit stack, big-integer decimals) takes the rows the first one deferred, as pjson_kernels.inc does.
// Every loop is bounded by a length (never by a sentinel); nothing recurses.  Included inside namespace flbgpu after kdev.inc,
// lane_rows.inc and canon_walk.inc.

enum { KBM_UNSET = 0, KBM_NONE = 1, KBM_PARSED = 2, KBM_MAP = 3 };

struct KbCfg {
    const LDS_AS uint32_t *w;       // the table's words in LDS
    uint32_t flags, key_bytes, tail_bytes;
};

// strncmp(p, word, len) == 0 for a word of six bytes: every prefix of the word, and a longer text only when a NUL follows the word
DEV bool kb_is_word(const uint8_t *p, uint32_t len, const char *word) {
    const uint32_t n = len < 6 ? len : 6;
    for (uint32_t i = 0; i < n; i++) if (ld8(p + i) != (uint32_t) (uint8_t) word[i]) return false;
    return len <= 6 || ld8(p + 6) == 0;
}

// value_trim_size (:139-161) over a text that goes by once, front to back: t = bytes of the longest tail that reads as a run of
// '\n', "\\n" and "\\r" (the reference walks it from the back; a byte decides its token alone, so both walks cut the same run).
// The reference's loop ends at i > 0: a '\n' that is the text's first byte stays.
struct KbTrimSink {
    uint32_t n = 0, t = 0, saved = 0, first = 0;
    bool bs = false;
    DEV void put(uint32_t b) {
        b &= 0xffu;
        if (n == 0) first = b;
        if (b == '\n') { t += 1; bs = false; }
        else if (b == '\\') { saved = t; t = 0; bs = true; }
        else if ((b == 'n' || b == 'r') && bs) { t = saved + 2; bs = false; }
        else { t = 0; bs = false; }
        n++;
    }
    DEV void put32(uint32_t w) { put(w); put(w >> 8); put(w >> 16); put(w >> 24); }
    DEV uint32_t size() const { return (t == n && n > 0 && first == '\n') ? 1u : n - t; }
};

// the first `left` bytes of what goes by
template <class S> struct KbCutSink {
    S &o;
    uint32_t left;
    DEV void put(uint32_t b) { if (left) { o.put(b); left--; } }
    DEV void put32(uint32_t w) { put(w & 255); put((w >> 8) & 255); put((w >> 16) & 255); put(w >> 24); }
};

// a top-level STR value whose opening quote is at i, cut by value_trim_size: STR header of the cut length + that many decoded bytes
template <class S> DEV uint32_t kb_trimmed_string(const JsonSrc &s, uint32_t i, S &o) {
    KbTrimSink ts;
    const uint32_t e = js_str_body(s, i + 1, ts);
    if (!e) return 0;
    const uint32_t keep = ts.size();
    pk_str_hdr(o, keep);
    if constexpr (std::is_same<S, JsonCountSink>::value) o.n += keep;
    else {
        KbCutSink<S> cut{o, keep};
        js_str_body(s, i + 1, cut);
    }
    return e;
}

// the pairs of the object whose '{' is at `open` into o (:498-528): "key": value, ... '}'.  Returns the position behind '}', 0 when
// the object is malformed or status became JS_DEFER.  max_open: most containers open at once inside a value.
template <bool EXACT, int NW, class S>
DEV uint32_t kb_pairs(const JsonSrc &s, uint32_t open, bool trim, S &o, uint32_t &npairs, int &status, uint32_t &max_open) {
    uint32_t i = open + 1;
    npairs = 0;
    while (js_ws(s[i])) i++;
    if (s[i] == '}') return i + 1;
    for (;;) {
        while (js_ws(s[i])) i++;
        if (s[i] != '"') return 0;
        uint32_t e = js_string(s, i, o);
        if (!e) return 0;
        i = e;
        while (js_ws(s[i])) i++;
        if (s[i] != ':') return 0;
        i++;
        while (js_ws(s[i])) i++;
        if (s[i] == '"') e = trim ? kb_trimmed_string(s, i, o) : js_string(s, i, o);
        else {
            JsonCounts cc;
            cc.col = nullptr; cc.n = 0; cc.r = 0; cc.next = JSON_CNT_SLOTS; cc.max_open = 0; cc.store = false;      // no columns: every count is looked up ahead
            int rt = 0;
            e = js_value<EXACT, NW>(s, i, o, rt, status, cc);
            if (cc.max_open > max_open) max_open = cc.max_open;
        }
        if (!e) return 0;
        i = e;
        npairs++;
        while (js_ws(s[i])) i++;
        if (s[i] == ',') { i++; continue; }
        if (s[i] == '}') return i + 1;
        return 0;
    }
}

struct KbMerge {
    int status = KBM_UNSET;
    bool defer = false;
    uint32_t open = 0;          // KBM_PARSED: where the object begins
    bool empty = false;         // KBM_PARSED: the packed map does not unpack again (:405-412, KB_UNPACK_OPEN): no entries
};

// merge_log_handler's default branch (:222-246) on a STR: flb_pack_json_recs answers one record that is an object, or nothing is merged
template <bool EXACT, int NW> DEV KbMerge kb_try_json(const uint8_t *v, uint32_t vlen, bool trim) {
    KbMerge m;
    m.status = KBM_NONE;
    JsonSrc s;
    s.p = v; s.len = vlen;
    uint32_t i = 0;
    while (i < vlen && js_ws(s[i])) i++;
    if (i >= vlen || s[i] != '{') return m;
    JsonCountSink cs;
    int status = JS_OK;
    uint32_t np = 0, max_open = 0;
    const uint32_t e = kb_pairs<EXACT, NW>(s, i, trim, cs, np, status, max_open);
    // (with the wide stack: deeper than 4096 levels -- the value counts as unparsable, nothing is merged)
    if (status == JS_DEFER) { m.defer = !EXACT; return m; }
    if (!e) return m;
    uint32_t q = e;
    while (q < vlen && js_ws(s[q])) q++;
    if (q < vlen) {
        // whatever follows must not parse as a second value (records != 1, :233-239)
        JsonNullSink ns;
        JsonCounts c2;
        c2.col = nullptr; c2.n = 0; c2.r = 0; c2.next = JSON_CNT_SLOTS; c2.max_open = 0; c2.store = false;
        int rt = 0, st2 = JS_OK;
        const uint32_t e2 = js_value<EXACT, NW>(s, q, ns, rt, st2, c2);
        if (st2 == JS_DEFER) { m.defer = !EXACT; return m; }
        if (e2) return m;
    }
    m.status = KBM_PARSED;
    m.open = i;
    m.empty = max_open >= KB_UNPACK_OPEN || np == 0;
    return m;
}

struct KbRow {
    bool bad = false, defer = false, seen = false, excluded = false, merged = false, odd = false, late = false;
    uint8_t sized = 0;          // size pass: KBS_PARSED / KBS_EMPTY for the emit pass
    uint64_t len = 0;           // size pass: output bytes without the tail; 0: nothing goes out
};

// one record into s (:318-584, without the tail).  false: the row is not one well-formed event
template <bool EXACT, int NW, class S>
DEV bool kb_record(const KbCfg &cf, const Event &ev, const uint8_t *end, uint32_t log_index, const KbMerge &m, const uint8_t *log_val, uint32_t log_len, S &s) {
    put_event_head(s, (uint32_t) ev.sec, (uint32_t) ev.nsec);
    // (the metadata is never set: the encoder's dynamic field closes as an empty map32, like the body's header)
    s.put(0xdf);
    s.put32(0);
    const bool keep_log = (cf.flags & KBF_KEEP_LOG) != 0, trim = (cf.flags & KBF_TRIM) != 0;
    const Tok bm = mp_tok(ev.body, end);
    uint8_t *hdr = open_map32(s);
    uint64_t entries = 0;
    const uint8_t *merged_map = nullptr;
    const bool whole = put_entries(s, bm, end, [&](uint32_t i, const uint8_t *, const uint8_t *v) {
        if (i == log_index) {
            if (m.status == KBM_MAP) merged_map = v;
            if (keep_log && (m.status == KBM_NONE || m.status == KBM_PARSED)) { entries++; return ENTRY_OWN; }
            if (!(keep_log || m.status == KBM_NONE)) return ENTRY_DROP;     // merged and keep_log off -- or a value of another type (:452)
        }
        entries++;
        return ENTRY_KEEP;
    }, [&](uint32_t, const uint8_t *e0, const uint8_t *) {
        // `log` kept beside what it merged into: the key as it is packed again, the value as a STR of the same bytes (:442-446)
        mp_canon(e0, end, s, 2);
        pk_str_hdr(s, log_len);
        put_span(s, log_val, log_len);
    });
    if (!whole) return false;
    // the merged pairs, in place or under merge_log_key (:474-584): the key only when there is at least one entry
    uint64_t inner = 0;
    uint8_t *ihdr = nullptr;
    const bool nest = (cf.flags & KBF_MERGE_KEY) != 0;
    if (m.status == KBM_PARSED && !m.empty) {
        if (nest) { put_lds(s, cf.w + KB_HDR_WORDS, cf.key_bytes); ihdr = open_map32(s); }
        JsonSrc js;
        js.p = log_val; js.len = log_len;
        uint32_t np = 0, mo = 0;
        int status = JS_OK;
        if constexpr (std::is_same<S, CountSink>::value) {
            JsonCountSink o;
            kb_pairs<EXACT, NW>(js, m.open, trim, o, np, status, mo);
            s.n += o.n;
        }
        else kb_pairs<EXACT, NW>(js, m.open, trim, s, np, status, mo);
        inner = np;
    }
    else if (m.status == KBM_MAP) {
        const Tok mt = mp_tok(merged_map, end);
        if (mt.len) {
            if (nest) { put_lds(s, cf.w + KB_HDR_WORDS, cf.key_bytes); ihdr = open_map32(s); }
            const uint8_t *q = mt.next;
            for (uint32_t i = 0; i < 2 * mt.len; i++) { q = mp_canon(q, end, s, 3); if (!q) return false; }
            inner = mt.len;
        }
    }
    if (inner) {
        if (nest) { close_map32(s, ihdr, inner); entries++; }
        else entries += inner;
    }
    // (the tail's pairs -- kubernetes, kubernetes_namespace -- are part of the body)
    close_map32(s, hdr, entries + ((cf.flags >> KBF_TAIL_PAIRS_SHIFT) & 3u));
    return true;
}

// decides one row: the decoder, the stream and the exclusion (:733-806), the time (:383-400), `log` (:348-380).  SIZE: its length.
template <bool EXACT, int NW, int PASS, class S>
DEV KbRow kb_row(const KbCfg &cf, const uint8_t *rec, const uint8_t *end, S &s, uint8_t sized = 0) {
    KbRow w;
    if (rec == end) return w;                                           // a record an earlier filter dropped
    const Event ev = decode_event(rec, end, false);
    if ((ev.flags & RF_BAD) || ev.body_end != end) { w.bad = true; return w; }
    if (ev.flags & RF_SKIP) return w;                                   // group markers and negative times: the decoder steps over them
    w.seen = true;
    const Tok bm = mp_tok(ev.body, end);
    // get_stream: the first STR key that strncmp calls "stream" decides
    int stream = 0;                                                     // 0 none, 1 stdout, 2 stderr, 3 unknown
    uint32_t log_index = 0xffffffffu, log_len = 0;
    const uint8_t *log_val = nullptr;
    int log_type = T_BAD;
    bool odd_key = false;
    const bool merge_log = (cf.flags & KBF_MERGE_LOG) != 0;
    const uint8_t *p = bm.next;
    for (uint32_t i = 0; i < bm.len; i++) {
        const Tok kt = mp_tok(p, end);
        const uint8_t *kend = mp_end_of(kt, p, end);
        const Tok vt = mp_tok(kend, end);
        p = mp_end_of(vt, kend, end);
        if (stream == 0 && kt.type == T_STR && kb_is_word(kt.next, kt.len, "stream")) {
            if (vt.type == T_STR || vt.type == T_BIN)
                stream = kb_is_word(vt.next, vt.len, "stdout") ? 1 : kb_is_word(vt.next, vt.len, "stderr") ? 2 : 3;
            else { stream = 3; w.odd = true; }                          // (the reference reads another member of the union)
        }
        if (merge_log && log_index == 0xffffffffu) {
            // :353: the size and the bytes of the key, whatever its type -- STR and BIN share the layout
            if ((kt.type == T_STR || kt.type == T_BIN) && kt.len == 3 && ld8(kt.next) == 'l' && ld8(kt.next + 1) == 'o' && ld8(kt.next + 2) == 'g') {
                log_index = i; log_type = vt.type; log_val = vt.type == T_MAP ? kend : vt.next; log_len = vt.len;
            }
            else if ((kt.type == T_UINT || kt.type == T_NINT || kt.type == T_F64) && (uint32_t) kt.u == 3) odd_key = true;   // (size 3 and a wild pointer)
        }
    }
    const bool ex_out = (cf.flags & KBF_EXCL_STDOUT) != 0, ex_err = (cf.flags & KBF_EXCL_STDERR) != 0;
    if ((stream == 1 && ex_out) || (stream == 2 && ex_err) || ((stream == 0 || stream == 3) && ex_out && ex_err)) { w.excluded = true; return w; }
    if (odd_key) w.odd = true;                                          // (an excluded record never reaches the lookup)
    if (encoder_refuses_time(ev.sec, ev.nsec)) { w.late = true; return w; }
    KbMerge m;
    if (log_index != 0xffffffffu) {
        if (log_type == T_MAP) m.status = KBM_MAP;
        else if (log_type == T_STR) {
            if constexpr (PASS == KB_EMIT) {
                // what the size pass decided stands in the row's state byte: the text is not walked a second time to decide it again
                m.status = (sized & KBS_PARSED) ? KBM_PARSED : KBM_NONE;
                m.empty = (sized & KBS_EMPTY) != 0;
                while (m.open < log_len && js_ws(ld8(log_val + m.open))) m.open++;
            }
            else {
                m = kb_try_json<EXACT, NW>(log_val, log_len, (cf.flags & KBF_TRIM) != 0);
                if (m.defer) { w.defer = true; return w; }
            }
        }
    }
    w.merged = m.status == KBM_PARSED || m.status == KBM_MAP;
    w.sized = (uint8_t) ((m.status == KBM_PARSED ? KBS_PARSED : 0) | (m.empty ? KBS_EMPTY : 0));
    if (!kb_record<EXACT, NW, S>(cf, ev, end, log_index, m, log_val, log_len, s)) { w.bad = true; return w; }
    if constexpr (PASS == KB_SIZE) w.len = s.n;
    return w;
}

// the tail behind one record, by the whole wave: byte stores up to the first dword boundary of the destination, dword stores, byte
// stores for what is left.  Every store lies in [dst, dst + n).
template <class SRC> DEV void kb_append(uint8_t *dst, SRC src, uint32_t n, uint32_t lane) {
    typedef uint32_t u32u __attribute__((aligned(1)));
    uint32_t head = (uint32_t) ((4u - ((uint32_t) (uintptr_t) dst & 3u)) & 3u);
    if (head > n) head = n;
    const uint32_t nd = (n - head) >> 2, rest = (n - head) & 3u;
    if (lane < head) dst[lane] = src[lane];
    uint32_t *d4 = (uint32_t *) (dst + head);
    for (uint32_t k = lane; k < nd; k += 64) {
        if constexpr (std::is_same<SRC, const LDS_AS uint8_t *>::value) d4[k] = *(const LDS_AS u32u *) (src + head + 4 * k);
        else d4[k] = *(const u32u *) (src + head + 4 * k);
    }
    if (lane < rest) dst[head + 4 * nd + lane] = src[head + 4 * nd + lane];
}

template <int PASS, bool EXACT>
__global__ void __launch_bounds__(KB_BLOCK) k_kube(KubeArgs a) {
    constexpr int NW = EXACT ? JSON_GENERIC_WORDS : 1;
    LDS_AS uint32_t *lds = lane_stage_table<KB_BLOCK>(a.table, a.table_bytes);
    LDS_AS uint8_t *tail_lds = (LDS_AS uint8_t *) g_lds + a.table_bytes;
    if (PASS == KB_EMIT && a.tail_in_lds) for (uint32_t i = threadIdx.x; i < a.tail_bytes; i += KB_BLOCK) tail_lds[i] = a.tail[i];
    __syncthreads();
    KbCfg cf;
    cf.w = lds; cf.flags = lds[0]; cf.key_bytes = lds[1]; cf.tail_bytes = a.tail_bytes;
    const uint32_t T = a.tail_bytes;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long n_seen = 0, n_merged = 0, n_excl = 0, n_odd = 0, n_out = 0, n_big = 0, n_mis = 0, n_defer = 0;
    // (the tail's ballot and shuffles below need the whole wave in every trip)
    lane_wave_rows<KB_BLOCK>(a.n, [&](uint64_t r, bool live) {
        uint8_t st = 0;
        if (live && (PASS == KB_EMIT || EXACT)) st = a.state[r];
        const bool mine = live && (EXACT ? (st & KBS_DEFER) != 0 : true);
        const uint8_t *rec = nullptr, *end = nullptr;
        if (mine) { rec = a.data + a.row_off[r]; end = a.data + a.row_off[r + 1]; }
        if (PASS == KB_EMIT) {
            const bool writes = mine && (st & KBS_OUT) && (EXACT || !(st & KBS_DEFER));
            uint64_t tail_at = 0;
            if (writes) {
                uint8_t *o0 = a.out + a.out_off[r], *o1 = a.out + a.out_off[r + 1];
                tail_at = a.out_off[r + 1] - T;
                BoundedSink bs(o0, o1 - T);
                const KbRow w = kb_row<EXACT, NW, KB_EMIT>(cf, rec, end, bs, st);
                if (w.bad || w.defer || bs.over || bs.p != o1 - T) n_mis++;
            }
            // the tail: one record after the other, 64 lanes each
            unsigned long long todo = T ? __ballot(writes) : 0ull;
            while (todo) {
                const int j = __ffsll((long long) todo) - 1;
                todo &= todo - 1;
                uint8_t *dst = a.out + __shfl(tail_at, j, 64);
                if (a.tail_in_lds) kb_append<const LDS_AS uint8_t *>(dst, tail_lds, T, lane);
                else kb_append<const uint8_t *>(dst, a.tail, T, lane);
            }
            return;
        }
        if (!mine) return;
        CountSink cs;
        KbRow w = kb_row<EXACT, NW, KB_SIZE>(cf, rec, end, cs);
        if (w.defer) { a.state[r] = KBS_DEFER; a.len[r] = 0; n_defer++; return; }        // (never under EXACT)
        uint64_t len = 0;
        if (w.bad) atomicMin(&a.firsts[0], (unsigned long long) r);
        else {
            if (w.late) atomicMin(&a.firsts[1], (unsigned long long) r);
            if (w.seen) n_seen++;
            if (w.excluded) n_excl++;
            if (w.odd) n_odd++;
            if (w.len) {
                len = w.len + T;
                if (len > 0xFFFFFFFFull || (uint64_t) (end - rec) > 0xFFFFFFFFull) { n_big++; len = 0; }      // a row the u32 column cannot hold
                else { n_out++; if (w.merged) n_merged++; }
            }
        }
        a.len[r] = (uint32_t) len;
        a.state[r] = (uint8_t) ((len ? KBS_OUT : 0) | (EXACT ? KBS_DEFER : 0) | w.sized);
    });
    if (PASS == KB_EMIT) { lane_flush(&a.counts[6], n_mis); return; }
    lane_flush(&a.counts[0], n_seen); lane_flush(&a.counts[1], n_merged); lane_flush(&a.counts[2], n_excl); lane_flush(&a.counts[3], n_odd);
    lane_flush(&a.counts[4], n_out); lane_flush(&a.counts[5], n_big); lane_flush(&a.counts[7], n_defer);
}

void launch_kube(const KubeArgs &a, int pass, bool exact, hipStream_t st) {
    if (a.n == 0) return;
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        const void *ks[] = {(const void *) k_kube<KB_SIZE, false>, (const void *) k_kube<KB_SIZE, true>, (const void *) k_kube<KB_EMIT, false>,
                            (const void *) k_kube<KB_EMIT, true>};
        for (const void *k : ks) (void) hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        attr_set = true;
    }
    const dim3 g(lane_blocks<KB_BLOCK>(a.n)), b(KB_BLOCK);
    const size_t lds = a.table_bytes + (a.tail_in_lds ? a.tail_bytes : 0);
    if (pass == KB_EMIT) {
        if (exact) hipLaunchKernelGGL((k_kube<KB_EMIT, true>), g, b, lds, st, a);
        else hipLaunchKernelGGL((k_kube<KB_EMIT, false>), g, b, lds, st, a);
    }
    else if (exact) hipLaunchKernelGGL((k_kube<KB_SIZE, true>), g, b, lds, st, a);
    else hipLaunchKernelGGL((k_kube<KB_SIZE, false>), g, b, lds, st, a);
}
