// sp_kernels.inc -- the stream processor's GROUP BY aggregation on the device (included by kernels_l2m.hip after
// l2m_kernels.inc, namespace flbgpu): what sp_process_data_aggr (src/stream_processor/flb_sp.c:1435-1601) does to one chunk.
//
//   k_sp_extract    one record per lane out of LDS-staged tiles: WHERE (reduce_expression :1011-1159 as a postfix program over
//                   leaf comparisons, the bool stack a bit mask), GROUP BY values -> canonical typed tuple -> group id through
//                   the device dictionary (sp_process_aggregate_data :1280-1429 + the rb-tree), aggregated keys -> typed
//                   number columns (object_to_number :361-401).  Touches no aggregate.
//   k_sp_aggregate  columns -> group rows: counts, wrapping int64 sums, exact fixed-point sums, min / max as order-preserving
//                   unsigned words -- integer max / add only, combined per workgroup in an LDS hash table first
//   k_sp_normalize  carry propagation of the sum digits
//
// Everything order-dependent in the reference (first-seen group order, the I64 -> F64 switch of a sum at the first non-zero
// float, sequential float addition) is recovered on the host from these order-independent words (sp.cpp).

enum { SV_NONE = 0, SV_NULL, SV_BOOL, SV_INT, SV_FLOAT, SV_STR };
struct SpVal {
    int type;            // SV_*: the expression value class (flb_sp_key.c:54-101); SV_NONE = no value (NULL pointer in the reference)
    int raw;             // T_* of the msgpack object behind it
    uint64_t u;          // int64 bits / binary64 bits / bool
    const uint8_t *s;
    uint32_t len;
};

DEV bool sp_name_eq(const uint8_t *p, uint32_t len, const char *name, uint32_t nlen) {
    if (len != nlen) return false;
    for (uint32_t i = 0; i < len; i++) if (ld8(p + i) != (uint32_t) (uint8_t) name[i]) return false;
    return true;
}

DEV SpVal sp_value_of(const uint8_t *v, const uint8_t *end) {
    SpVal r;
    r.type = SV_NONE; r.raw = T_BAD; r.u = 0; r.s = nullptr; r.len = 0;
    Tok t = mp_tok(v, end);
    r.raw = t.type;
    switch (t.type) {
    case T_BOOL: r.type = SV_BOOL; r.u = t.u ? 1 : 0; break;
    case T_UINT: case T_NINT: r.type = SV_INT; r.u = t.u; break;
    case T_F32: r.type = SV_FLOAT; r.u = (uint64_t) __double_as_longlong((double) __uint_as_float((uint32_t) t.u)); break;
    case T_F64: r.type = SV_FLOAT; r.u = t.u; break;
    case T_STR: r.type = SV_STR; r.s = t.next; r.len = t.len; break;
    case T_MAP: r.type = SV_BOOL; r.u = 1; break;                 // "just denoting the existence of the key"
    case T_NIL: r.type = SV_NULL; break;
    default: break;                                               // array / bin / ext: no value
    }
    return r;
}

// flb_sp_key_to_value (flb_sp_key.c:161-222): the FIRST entry of the body whose key is `name`; sub-keys walk nested maps
// (subkey_to_value :103-159), first match at every level; a non-map value ignores the sub-keys.  *count = entries named `name`
// (the callers' loops run once per such entry): *count the string entries (a map32 holds fewer than 2^32: it cannot wrap), *bins
// the bin-typed ones, which only the GROUP BY loop's `found` asks about -- a sum it compares with at most SP_MAX_GB, so they are
// counted up to SP_BINS_MAX and no further.
constexpr uint32_t SP_BINS_MAX = 7;
DEV SpVal sp_lookup(const SpPlan *pl, const SpKeyRef &k, const uint8_t *map, const uint8_t *end, uint32_t *count, uint32_t *bins) {
    SpVal none;
    none.type = SV_NONE; none.raw = T_BAD; none.u = 0; none.s = nullptr; none.len = 0;
    *count = 0; *bins = 0;
    Tok m = mp_tok(map, end);
    if (m.type != T_MAP) return none;
    const uint8_t *p = m.next, *first = nullptr;
    uint32_t cnt = 0, nb = 0;
    for (uint32_t i = 0; i < m.len; i++) {
        Tok kk = mp_tok(p, end);
        const uint8_t *v = mp_skip(p, end, 2);
        if (!v) break;
        // (flb_sp_key_to_value compares key.via.str without a look at key.type, flb_sp_key.c:189, and bin shares the layout: the value
        // is the first str-or-bin entry's.  *count: string entries (the loop over the select keys wants key.type == STR,
        // flb_sp.c:1510), *bins: binary ones (the GROUP BY loop :1317-1326 does not look at the type either)
        if ((kk.type == T_STR || kk.type == T_BIN) && sp_name_eq(kk.next, kk.len, pl->blob + k.name_off, k.name_len)) {
            if (!first) first = v;
            if (kk.type == T_STR) cnt++;
            else if (nb < SP_BINS_MAX) nb++;
        }
        p = mp_skip(v, end, 2);
        if (!p) break;
    }
    *count = cnt; *bins = nb;
    if (!first) return none;
    Tok t = mp_tok(first, end);
    if (t.type == T_MAP && k.nsub > 0) {
        const uint8_t *cur = first;
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
                if (!v) return none;
                if (kk.type == T_STR && sp_name_eq(kk.next, kk.len, pl->blob + k.sub_off[lv], k.sub_len[lv])) { found = true; cur = v; matched++; break; }
                q = mp_skip(v, end, 3);
                if (!q) return none;
            }
            if (matched == k.nsub) break;
        }
        if (!found || (matched > 0 && matched != k.nsub)) return none;
        return sp_value_of(cur, end);
    }
    return sp_value_of(first, end);
}

// ---- one walk for all keys of the plan: the first value and the number of entries per key reference (plans with at most
// SP_FAST_KEYS distinct keys; larger ones look every key up with its own walk)
constexpr int SP_FAST_KEYS = 6;
struct SpHits {
    bool fast;
    const uint8_t *first[SP_FAST_KEYS];
    uint32_t cnt[SP_FAST_KEYS];                                   // string entries per key, as sp_lookup's *count
    uint32_t bins;                                                // bin-typed entries, four bits per key, each pinned at SP_BINS_MAX
};
// false: the body does not decode.  *walk_end = first byte after the map
DEV bool sp_walk(const SpPlan *pl, const uint8_t *map, const uint8_t *end, SpHits &h, const uint8_t **walk_end) {
    #pragma unroll
    for (int k = 0; k < SP_FAST_KEYS; k++) { h.first[k] = nullptr; h.cnt[k] = 0; }
    h.bins = 0;
    Tok m = mp_tok(map, end);
    if (m.type != T_MAP) return false;
    const uint8_t *p = m.next;
    const int nk = pl->nkeys;
    for (uint32_t i = 0; i < m.len; i++) {
        Tok kk = mp_tok(p, end);
        const uint8_t *v = mp_end_of(kk, p, end, 2);
        if (!v) return false;
        if (kk.type == T_STR || kk.type == T_BIN) {
            #pragma unroll
            for (int k = 0; k < SP_FAST_KEYS; k++) {
                if (k < nk && kk.len == pl->keys[k].name_len && sp_name_eq(kk.next, kk.len, pl->blob + pl->keys[k].name_off, kk.len)) {
                    if (!h.first[k]) h.first[k] = v;
                    if (kk.type == T_STR) h.cnt[k]++;
                    else if (((h.bins >> (4 * k)) & 15u) < SP_BINS_MAX) h.bins += 1u << (4 * k);
                }
            }
        }
        Tok vt = mp_tok(v, end);
        p = mp_end_of(vt, v, end, 2);
        if (!p) return false;
    }
    *walk_end = p;
    return true;
}

// the value behind the first entry of a key (sub-keys resolved): the second half of sp_lookup
DEV SpVal sp_first_value(const SpPlan *pl, const SpKeyRef &k, const uint8_t *first, const uint8_t *end) {
    SpVal none;
    none.type = SV_NONE; none.raw = T_BAD; none.u = 0; none.s = nullptr; none.len = 0;
    if (!first) return none;
    Tok t = mp_tok(first, end);
    if (t.type == T_MAP && k.nsub > 0) {
        const uint8_t *cur = first;
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
                if (!v) return none;
                if (kk.type == T_STR && sp_name_eq(kk.next, kk.len, pl->blob + k.sub_off[lv], k.sub_len[lv])) { found = true; cur = v; matched++; break; }
                q = mp_skip(v, end, 3);
                if (!q) return none;
            }
            if (matched == k.nsub) break;
        }
        if (!found || (matched > 0 && matched != k.nsub)) return none;
        return sp_value_of(cur, end);
    }
    return sp_value_of(first, end);
}

DEV SpVal sp_get(const SpPlan *pl, const SpHits &h, uint32_t key, const uint8_t *map, const uint8_t *end, uint32_t *count, uint32_t *bins) {
    if (!h.fast) return sp_lookup(pl, pl->keys[key], map, end, count, bins);
    const uint8_t *f = h.first[0];
    uint32_t c = h.cnt[0];
    #pragma unroll
    for (int k = 1; k < SP_FAST_KEYS; k++) if (key == (uint32_t) k) { f = h.first[k]; c = h.cnt[k]; }
    *count = c;
    *bins = (h.bins >> (4 * key)) & 15u;
    return sp_first_value(pl, pl->keys[key], f, end);
}

// string_to_number (flb_sp.c:264-357): 0 not a number, 1 integer (strtoll), 2 float (strtold narrowed to double).
// '.' is counted over all len bytes, the conversions stop at the first NUL like the C functions.
// GENERIC = false: a string with one '.' is not converted here (the exact decimal -> binary64 conversion is heavy): *defer is
// set and the record goes to the generic instantiation of the kernel
template <bool GENERIC>
DEV int sp_str_to_num(const uint8_t *s, uint32_t len, int64_t *iv, uint64_t *fbits, unsigned int *flags, bool *defer) {
    uint32_t dots = 0, z = len;
    for (uint32_t i = 0; i < len; i++) {
        uint32_t c = ld8(s + i);
        if (c == '.') dots++;
        if (c == 0 && z == len) z = i;
    }
    if (dots > 1) return 0;
    len = z;
    if (dots == 1) {
        if constexpr (!GENERIC) { *defer = true; return 0; }
        L2mPtrSrc src{s};
        nc::ScanResult r = nc::scan_double<true>(src, len, nc::MODE_STRTOD);
        if (r.status != nc::NC_OK || r.consumed == 0) return 0;
        const uint64_t mag = r.bits & ~nc::DBL_SIGN;
        if (mag == nc::DBL_INF_BITS || mag == 0) {
            // strtold's range is wider than binary64's: out-of-range decimals with up to three exponent digits are inside it
            // (they narrow to inf / 0); longer exponents may be ERANGE there -- not decided here
            uint32_t i = 0, ed = 0;
            while (i < len && d_lower(ld8(s + i)) != 'e' && d_lower(ld8(s + i)) != 'p') i++;
            if (i < len) { i++; if (i < len && (ld8(s + i) == '+' || ld8(s + i) == '-')) i++; while (i < len && d_isdigit(ld8(s + i))) { ed++; i++; } }
            if (ed >= 4) atomicOr(flags, (unsigned int) SPF_FLOAT_RANGE);
        }
        *fbits = r.bits;
        return 2;
    }
    uint32_t i = 0;
    while (i < len && d_isspace(ld8(s + i))) i++;
    bool neg = false;
    if (i < len && (ld8(s + i) == '-' || ld8(s + i) == '+')) { neg = ld8(s + i) == '-'; i++; }
    if (i >= len || !d_isdigit(ld8(s + i))) return 0;
    uint64_t acc = 0;
    const uint64_t lim = neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull;
    for (; i < len && d_isdigit(ld8(s + i)); i++) {
        const uint64_t dgt = ld8(s + i) - '0';
        if (acc > (lim - dgt) / 10) return 0;                     // ERANGE
        acc = acc * 10 + dgt;
    }
    *iv = neg ? (int64_t) (0 - acc) : (int64_t) acc;
    return 1;
}

// strncmp(l, r, l.len) over NUL-terminated buffers (flb_sds strings carry the terminator)
DEV int sp_strncmp(const SpVal &l, const SpVal &r) {
    for (uint32_t i = 0; i < l.len; i++) {
        const uint32_t ca = ld8(l.s + i), cb = i < r.len ? ld8(r.s + i) : 0;
        if (ca != cb) return (int) ca - (int) cb;
        if (ca == 0) return 0;
    }
    return 0;
}

// numerical_comp (flb_sp.c:783-960)
template <bool GENERIC>
DEV bool sp_compare(int op, SpVal l, SpVal r, unsigned int *flags, bool *defer) {
    if (l.type == SV_NONE || r.type == SV_NONE) return false;
    if (l.type == SV_STR && r.type != SV_STR) {
        int64_t iv = 0;
        uint64_t fb = 0;
        const int k = sp_str_to_num<GENERIC>(l.s, l.len, &iv, &fb, flags, defer);
        if (k == 1) { l.type = SV_INT; l.u = (uint64_t) iv; }
        else if (k == 2) { l.type = SV_FLOAT; l.u = fb; }
    }
    if (l.type == SV_INT && r.type == SV_FLOAT) { l.type = SV_FLOAT; l.u = (uint64_t) __double_as_longlong((double) (int64_t) l.u); }
    else if (l.type == SV_FLOAT && r.type == SV_INT) { r.type = SV_FLOAT; r.u = (uint64_t) __double_as_longlong((double) (int64_t) r.u); }
    if (l.type != r.type) return false;
    if (l.type == SV_INT) {
        const int64_t a = (int64_t) l.u, b = (int64_t) r.u;
        return op == SPO_EQ ? a == b : op == SPO_LT ? a < b : op == SPO_LTE ? a <= b : op == SPO_GT ? a > b : a >= b;
    }
    if (l.type == SV_FLOAT) {
        const double a = __longlong_as_double((long long) l.u), b = __longlong_as_double((long long) r.u);
        return op == SPO_EQ ? a == b : op == SPO_LT ? a < b : op == SPO_LTE ? a <= b : op == SPO_GT ? a > b : a >= b;
    }
    if (l.type == SV_STR) {
        const int c = sp_strncmp(l, r);
        if (op == SPO_EQ) return l.len == r.len && c == 0;
        return op == SPO_LT ? c < 0 : op == SPO_LTE ? c <= 0 : op == SPO_GT ? c > 0 : c >= 0;
    }
    if (op != SPO_EQ) return false;
    if (l.type == SV_NULL) return true;
    return (l.u != 0) == (r.u != 0);                              // SV_BOOL
}

DEV SpVal sp_leaf(const SpPlan *pl, const SpHits &h, uint32_t li, const uint8_t *map, const uint8_t *end, double ts) {
    const SpLeaf &lf = pl->leaf[li];
    SpVal r;
    r.type = SV_NONE; r.raw = T_BAD; r.u = lf.v; r.s = nullptr; r.len = 0;
    uint32_t cnt, bins;
    switch (lf.kind) {
    case SPL_KEY: return sp_get(pl, h, lf.key, map, end, &cnt, &bins);
    case SPL_INT: r.type = SV_INT; break;
    case SPL_FLOAT: r.type = SV_FLOAT; break;
    case SPL_STR: r.type = SV_STR; r.s = (const uint8_t *) pl->blob + lf.str_off; r.len = lf.str_len; break;
    case SPL_BOOL: r.type = SV_BOOL; break;
    case SPL_NULL: r.type = SV_NULL; break;
    case SPL_TIME: r.type = SV_FLOAT; r.u = (uint64_t) __double_as_longlong(ts); break;
    case SPL_CONTAINS: {                                          // cb_contains: NULL in, NULL out; else true
        SpVal v = sp_get(pl, h, lf.key, map, end, &cnt, &bins);
        if (v.type != SV_NONE) { r.type = SV_BOOL; r.u = 1; }
        break;
    }
    default: break;
    }
    return r;
}

DEV bool sp_truth(const SpVal &v) {                               // value_to_bool (flb_sp.c:962-982); NULL pointer: false
    switch (v.type) {
    case SV_BOOL: return v.u != 0;
    case SV_INT: return (int64_t) v.u > 0;
    case SV_FLOAT: return __longlong_as_double((long long) v.u) > 0;
    case SV_STR: return true;
    default: return false;
    }
}

template <bool GENERIC>
DEV bool sp_where(const SpPlan *pl, const SpHits &h, const uint8_t *map, const uint8_t *end, double ts, unsigned int *flags, bool *defer) {
    uint32_t stk = 0;                                             // bit i = i-th entry from the bottom
    int sp = 0;
    for (int i = 0; i < pl->nops; i++) {
        const SpOp o = pl->ops[i];
        if (o.op <= SPO_GTE) {
            const bool b = sp_compare<GENERIC>(o.op, sp_leaf(pl, h, o.l, map, end, ts), sp_leaf(pl, h, o.r, map, end, ts), flags, defer);
            stk = (stk & ~(1u << sp)) | ((b ? 1u : 0u) << sp); sp++;
        }
        else if (o.op == SPO_TRUTH) {
            const bool b = sp_truth(sp_leaf(pl, h, o.l, map, end, ts));
            stk = (stk & ~(1u << sp)) | ((b ? 1u : 0u) << sp); sp++;
        }
        else if (o.op == SPO_NOT) stk ^= 1u << (sp - 1);
        else {
            const uint32_t b = (stk >> (sp - 1)) & 1, a = (stk >> (sp - 2)) & 1;
            const uint32_t r = o.op == SPO_AND ? (a & b) : (a | b);
            sp--;
            stk = (stk & ~(1u << (sp - 1))) | (r << (sp - 1));
        }
    }
    return sp > 0 ? ((stk >> (sp - 1)) & 1) != 0 : true;
}

// ---- the GROUP BY tuple: per column a class byte and its payload (int64 / canonical binary64 little-endian, or the string's
// bytes and a NUL); classes: 'i' ints, bools, numeric strings, and the zeroed slot of maps / nil; 'f'; 's'
struct SpTuple {
    int n;
    int cls[SP_MAX_GB];
    uint64_t u[SP_MAX_GB];
    const uint8_t *s[SP_MAX_GB];
    uint32_t len[SP_MAX_GB];
    template <class Sink> DEV void run(Sink &k) const {
        #pragma unroll
        for (int g = 0; g < SP_MAX_GB; g++) {
            if (g >= n) break;
            k.put((uint32_t) cls[g]);
            if (cls[g] == 's') { for (uint32_t j = 0; j < len[g]; j++) k.put(ld8(s[g] + j)); k.put(0); }
            else { for (int b = 0; b < 8; b++) k.put((uint32_t) (u[g] >> (8 * b)) & 0xff); }
        }
    }
};

// group id of a tuple, inserting it when new: the dictionary protocol of l2m_series_id over the same table type
DEV uint32_t sp_group_id(const L2mTable &t, const SpTuple &tp) {
    L2mHashSink hs;
    tp.run(hs);
    const uint64_t h = l2m_mix(hs.h);
    const uint32_t klen = hs.n;
    uint64_t pos = h & t.cap_mask;
    uint64_t probes = 0;
    while (probes <= t.cap_mask) {
        unsigned long long cur = l2m_ld64(&t.slot_hash[pos]);
        if (cur == h) {
            uint32_t sid = l2m_ld32(&t.slot_sid[pos]);
            if (l2m_ld32(&t.key_len[sid]) == klen) {
                L2mCmpSink cs(t.arena + l2m_ld64(&t.key_off[sid]), klen);
                tp.run(cs);
                if (cs.eq && cs.n == klen) return sid;
            }
            pos = (pos + 1) & t.cap_mask; probes++;
        }
        else if (cur == 0) {
            if (atomicCAS(&t.slot_hash[pos], 0ull, 1ull) == 0ull) {
                const uint32_t padded = (klen + 7) & ~7u;
                uint32_t sid = 0;
                unsigned long long off = 0;
                if (!l2m_reserve(t, padded, &sid, &off)) {                     // (l2m_dev.inc: counters that only move forward)
                    atomicExch(t.overflow, 1u);
                    l2m_st64(&t.slot_hash[pos], 0ull);
                    return SP_GID_NONE;
                }
                L2mStoreSink ss(t.arena + off);
                tp.run(ss);
                ss.finish();
                l2m_st64(&t.key_off[sid], off);
                l2m_st32(&t.key_len[sid], klen);
                l2m_st64(&t.series_hash[sid], h);
                l2m_st32(&t.slot_sid[pos], sid);
                __threadfence();
                l2m_st64(&t.slot_hash[pos], h);
                return sid;
            }
        }
        else if (cur != 1) { pos = (pos + 1) & t.cap_mask; probes++; }
    }
    atomicExch(t.overflow, 1u);
    return SP_GID_NONE;
}

// object_to_number (flb_sp.c:361-401): 0 none, 1 int, 2 float
template <bool GENERIC>
DEV int sp_to_number(const SpVal &v, int conv, int64_t *iv, uint64_t *fb, unsigned int *flags, bool *defer) {
    if (v.raw == T_UINT || v.raw == T_NINT) { *iv = (int64_t) v.u; return 1; }
    if (v.raw == T_F32 || v.raw == T_F64) { *fb = v.u; return 2; }
    if (v.raw == T_STR && conv && v.len <= 19) return sp_str_to_num<GENERIC>(v.s, v.len, iv, fb, flags, defer);
    return 0;
}

template <bool GENERIC>
DEV void sp_record(const SpArgs &a, uint64_t r, const uint8_t *rec, const uint8_t *rec_end, uint32_t &n_in, uint32_t &n_defer, uint32_t &seen) {
    const SpPlan *pl = a.plan;
    uint32_t gid = SP_GID_NONE;
    bool defer = false;
    for (int s = 0; s < pl->nsrc; s++) a.vt_col[(uint64_t) s * a.n + r] = 0;
    SpHits h;
    h.fast = pl->nkeys <= SP_FAST_KEYS;
    Event ev = decode_event(rec, rec_end, h.fast);
    if (h.fast && (ev.flags & RF_VALID)) {
        // the walk that collects the keys also is the body's validation
        const uint8_t *we = nullptr;
        if (!sp_walk(pl, ev.body, rec_end, h, &we) || we != rec_end) ev.flags = RF_BAD;
    }
    if (!(ev.flags & RF_VALID)) {
        // not [time | [time, meta], map]: the reference reads root.via.array.ptr[1] as a map whatever it is
        if (mp_skip(rec, rec_end, 0) != rec_end) atomicMin(a.first_bad, (unsigned long long) r);
        else atomicOr(a.flags, (unsigned int) SPF_BAD_RECORD);
        a.gid_col[r] = gid;
        return;
    }
    const uint8_t *map = ev.body, *end = ev.body_end;
    // flb_time_to_double of what flb_time_pop_from_msgpack read (group markers carry 0xffffffff / 0xfffffffe seconds)
    const double ts = (double) (uint64_t) (ev.sec < 0 ? 0x100000000ll + ev.sec : ev.sec) + (double) ev.nsec / 1000000000.0;
    bool pass = pl->nops == 0 || sp_where<GENERIC>(pl, h, map, end, ts, a.flags, &defer);
    if (pass && !defer) {
        SpTuple tp;
        tp.n = pl->ngb;
        uint64_t found = 0;
        #pragma unroll
        for (int g = 0; g < SP_MAX_GB; g++) {
            tp.cls[g] = 'i'; tp.u[g] = 0; tp.s[g] = nullptr; tp.len[g] = 0;
            if (g >= pl->ngb) continue;
            uint32_t cnt = 0, bins = 0;
            SpVal v = sp_get(pl, h, pl->gb_key[g], map, end, &cnt, &bins);
            if (v.type == SV_NONE) continue;
            found += (uint64_t) cnt + bins;
            int64_t iv = 0;
            uint64_t fb = 0;
            const int k = sp_to_number<GENERIC>(v, pl->str_conv, &iv, &fb, a.flags, &defer);
            if (k == 1) tp.u[g] = (uint64_t) iv;
            else if (k == 2) {
                if ((fb & ~nc::DBL_SIGN) > nc::DBL_INF_BITS) atomicOr(a.flags, (unsigned int) SPF_KEY_NAN);
                tp.cls[g] = 'f'; tp.u[g] = (fb & ~nc::DBL_SIGN) == 0 ? 0 : fb;
            }
            else if (v.raw == T_STR) {
                tp.cls[g] = 's'; tp.s[g] = v.s; tp.len[g] = v.len;
                for (uint32_t j = 0; j < v.len; j++) if (ld8(v.s + j) == 0) { atomicOr(a.flags, (unsigned int) SPF_KEY_NUL); break; }
            }
            else if (v.raw == T_BOOL) tp.u[g] = v.u;
        }
        if (defer) { }
        else if (found < (uint64_t) pl->ngb) pass = false;
        else {
            if (pl->ngb > 0) {
                #pragma unroll
                for (int g = 0; g < SP_MAX_GB; g++) {
                    if (g >= pl->ngb) continue;
                    const unsigned int bit = tp.cls[g] == 'i' ? 1u : tp.cls[g] == 'f' ? 2u : 4u;
                    if ((__hip_atomic_load(a.col_class + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0) atomicOr(a.col_class + g, bit);
                }
                gid = sp_group_id(a.t, tp);
            }
            else gid = 0;                                         // no GROUP BY: the one node of the window
        }
    }
    // (a deferred record is redone from scratch by k_sp_generic; a dictionary entry it made here is the one it will find)
    if (pass && !defer && gid != SP_GID_NONE) {
        for (int s = 0; s < pl->nsrc && !defer; s++) {
            uint32_t cnt = 0, bins = 0;                             // (the string entries: the loop over the select keys)
            SpVal v = sp_get(pl, h, pl->src_key[s], map, end, &cnt, &bins);
            if (v.type == SV_NONE || cnt == 0) continue;
            int64_t iv = 0;
            uint64_t fb = 0;
            int k = sp_to_number<GENERIC>(v, pl->str_conv, &iv, &fb, a.flags, &defer);
            if (k == 0) continue;
            if (k == 2 && (fb & ~nc::DBL_SIGN) == 0) { k = 1; iv = 0; }     // dval == 0.0: the reference adds ival (0)
            a.val_col[(uint64_t) s * a.n + r] = k == 1 ? (uint64_t) iv : fb;
            seen |= k == 2 ? 2u : iv != 0 ? 1u : 0u;
            a.vt_col[(uint64_t) s * a.n + r] = (uint8_t) (k | ((cnt >= SP_VT_MANY ? SP_VT_MANY : cnt) << 2));
            if (cnt >= SP_VT_MANY) a.cnt_col[(uint64_t) s * a.n + r] = cnt;
        }
        if (!defer) n_in++;
    }
    if (defer) { n_defer++; a.gid_col[r] = SP_GID_DEFER; }
    else a.gid_col[r] = pass ? gid : SP_GID_NONE;
}

constexpr int SP_BLOCK = 256;
constexpr int SP_TILE = 18432;

__global__ void __launch_bounds__(SP_BLOCK) k_sp_extract(SpArgs a) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LDS_AS uint8_t *tile = (LDS_AS uint8_t *) g_lds + (size_t) wave * SP_TILE;
    const uint64_t wave_id = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    const uint8_t *data_end = a.data + a.bytes;
    uint32_t n_in = 0, n_defer = 0, seen = 0;
    for (uint64_t base = wave_id * 64; base < a.n; base += nwaves * 64) {
        const uint64_t r = base + lane;
        const uint32_t cnt = (uint32_t) ((a.n - base) < 64 ? (a.n - base) : 64);
        uint64_t o0 = 0, o1 = 0;
        if (lane < cnt) { o0 = a.row_off[r]; o1 = a.row_off[r + 1]; }
        uint32_t lo = 0;
        while (lo < cnt) {
            // as many whole records as fit the wave's tile, loaded 16 B per lane
            const uint64_t g0 = __shfl(o0, (int) lo, 64);
            const uint32_t align = (uint32_t) (g0 & 15);
            const bool fit = lane >= lo && lane < cnt && (o1 - g0 + align) <= (uint64_t) SP_TILE;
            const uint64_t mask = __ballot(fit) >> lo;
            uint32_t m = (~mask == 0) ? 64 - lo : (uint32_t) __builtin_ctzll(~mask);
            if (m > cnt - lo) m = cnt - lo;
            const bool direct = (m == 0);
            if (direct) m = 1;
            if (!direct) {
                const uint32_t total = (uint32_t) (__shfl(o1, (int) (lo + m - 1), 64) - g0) + align;
                const uint8_t *src = a.data + (g0 - align);
                typedef uint32_t v4 __attribute__((ext_vector_type(4)));
                for (uint32_t u = lane; u * 16 < total; u += 64) {
                    const uint8_t *p = src + (size_t) u * 16;
                    v4 v;
                    if (p + 16 <= data_end) v = *(const v4 *) p;
                    else {
                        uint32_t t4[4] = {0, 0, 0, 0};
                        for (int q = 0; q < 16 && p + q < data_end; q++) t4[q >> 2] |= (uint32_t) p[q] << (8 * (q & 3));
                        v.x = t4[0]; v.y = t4[1]; v.z = t4[2]; v.w = t4[3];
                    }
                    *(LDS_AS v4 *) (tile + (size_t) u * 16) = v;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
            if (lane >= lo && lane < lo + m) {
                if (o0 == o1) {                                   // a row an earlier filter emptied: nothing to unpack
                    a.gid_col[r] = SP_GID_NONE;
                    for (int s = 0; s < a.plan->nsrc; s++) a.vt_col[(uint64_t) s * a.n + r] = 0;
                }
                // (two call sites, round 6: every pointer of the second one comes from the tile, so its loads are LDS reads -- with ONE
                // call behind a select between the chunk and the tile they were flat loads through the aperture, a record's every byte)
                else if (direct) sp_record<false>(a, r, a.data + o0, a.data + o1, n_in, n_defer, seen);
                else {
                    LDS_AS const uint8_t *lrec = tile + align + (uint32_t) (o0 - g0);
                    sp_record<false>(a, r, (const uint8_t *) lrec, (const uint8_t *) (lrec + (uint32_t) (o1 - o0)), n_in, n_defer, seen);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            lo += m;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { n_in += __shfl_down(n_in, o, 64); n_defer += __shfl_down(n_defer, o, 64); seen |= __shfl_down(seen, o, 64); }
    if (lane == 0 && seen) atomicOr(a.seen, seen);
    if (lane == 0 && n_in) atomicAdd(&a.counts[0], (unsigned long long) n_in);
    if (lane == 0 && n_defer) atomicAdd(&a.counts[1], (unsigned long long) n_defer);
}

// the records k_sp_extract deferred (a numeric string with a decimal point somewhere on their path), one per lane from HBM
__global__ void __launch_bounds__(64) k_sp_generic(SpArgs a) {
    uint32_t n_in = 0, n_defer = 0, seen = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (uint64_t) gridDim.x * blockDim.x) {
        if (a.gid_col[r] != SP_GID_DEFER) continue;
        sp_record<true>(a, r, a.data + a.row_off[r], a.data + a.row_off[r + 1], n_in, n_defer, seen);
    }
    for (int o = 32; o > 0; o >>= 1) { n_in += __shfl_down(n_in, o, 64); seen |= __shfl_down(seen, o, 64); }
    if ((threadIdx.x & 63) == 0 && seen) atomicOr(a.seen, seen);
    if ((threadIdx.x & 63) == 0 && n_in) atomicAdd(&a.counts[0], (unsigned long long) n_in);
}

// order-preserving maps onto unsigned words
DEV unsigned long long sp_ord_i(int64_t v) { return (unsigned long long) v ^ 0x8000000000000000ull; }
DEV unsigned long long sp_ord_f(uint64_t bits) { return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull); }

// mult times v = M * 2^E (M < 2^64) into the fixed-point digits at `lrow` (a digit is below 2^32 and so is mult: the product of
// the two is what mult additions of the digit leave in the word)
DEV void sp_add_digits(L2mCombiner<false> &cb, uint64_t lrow, uint64_t M, int64_t E, bool neg, uint64_t mult) {
    const uint32_t s = (uint32_t) (E + 1074), j = s >> 5, sh = s & 31;
    const uint64_t lo = M << sh, hi = sh ? (M >> (64 - sh)) : 0;
    const uint64_t d0 = (lo & 0xFFFFFFFFull) * mult, d1 = (lo >> 32) * mult, d2 = (hi & 0xFFFFFFFFull) * mult, d3 = (hi >> 32) * mult;
    if (d0) cb.add(lrow + j, neg ? 0 - d0 : d0);
    if (d1) cb.add(lrow + j + 1, neg ? 0 - d1 : d1);
    if (d2) cb.add(lrow + j + 2, neg ? 0 - d2 : d2);
    if (d3) cb.add(lrow + j + 3, neg ? 0 - d3 : d3);
}

// the global index of every (group, aggregated key)'s first non-zero float, ahead of k_sp_aggregate: run for the chunks that hold
// both such floats and non-zero integers -- the integers ahead of it are the ones the reference added as an int64
__global__ void __launch_bounds__(256) k_sp_first_float(SpAggArgs a) {
    const uint64_t lim = *a.first_bad < a.n ? *a.first_bad : a.n;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < lim; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t gid = a.gid_col[i];
        if (gid == SP_GID_NONE) continue;
        const unsigned long long o = ~(a.idx_base + i);
        for (int s = 0; s < a.nsrc; s++) {
            if ((a.vt_col[(uint64_t) s * a.n + i] & 3) != 2) continue;
            unsigned long long *w = &a.rows[(uint64_t) gid * a.W + 1 + (uint64_t) SP_SRC_MAX * s + SP_M_FIRST_FLT];
            if (o > *w) atomicMax(w, o);
        }
    }
}

__global__ void __launch_bounds__(L2M_AGG_BLOCK) k_sp_aggregate(SpAggArgs a) {
    LDS_AS uint32_t *keys = (LDS_AS uint32_t *) g_lds;
    LDS_AS unsigned long long *vals = (LDS_AS unsigned long long *) (g_lds + L2M_AGG_SLOTS * 4);
    for (uint32_t s = threadIdx.x; s < L2M_AGG_SLOTS; s += blockDim.x) { keys[s] = 0; vals[s] = 0; }
    __syncthreads();
    L2mCombiner<false> cb{keys, vals, a.rows};
    const uint64_t lim = *a.first_bad < a.n ? *a.first_bad : a.n;
    const uint64_t W = (uint64_t) a.W, A = 1 + (uint64_t) SP_SRC_MAX * a.nsrc;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < lim; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t gid = a.gid_col[i];
        if (gid == SP_GID_NONE) continue;
        const uint64_t row = (uint64_t) gid * W;
        const uint64_t gidx = a.idx_base + i;
        if (~gidx > a.rows[row]) atomicMax(&a.rows[row], (unsigned long long) ~gidx);
        cb.add(row + A, 1);
        for (int s = 0; s < a.nsrc; s++) {
            const uint32_t vt = a.vt_col[(uint64_t) s * a.n + i];
            const uint32_t cls = vt & 3;
            if (!cls) continue;
            const uint64_t mult = (vt >> 2) == SP_VT_MANY ? a.cnt_col[(uint64_t) s * a.n + i] : (vt >> 2);
            const uint64_t v = a.val_col[(uint64_t) s * a.n + i];
            const uint64_t mx = row + 1 + (uint64_t) SP_SRC_MAX * s, base = row + A + 1 + (uint64_t) SP_SRC_ADD * s;
            if (cls == 1) {
                const int64_t iv = (int64_t) v;
                cb.add(base + SP_A_NINT, mult);
                cb.add(base + SP_A_ISUM, (unsigned long long) iv * mult);
                const unsigned long long o = sp_ord_i(iv);
                if (~o > a.rows[mx + 0]) atomicMax(&a.rows[mx + 0], ~o);
                if (o > a.rows[mx + 1]) atomicMax(&a.rows[mx + 1], o);
                if (iv != 0) {
                    const uint64_t M = iv < 0 ? (uint64_t) 0 - (uint64_t) iv : (uint64_t) iv;
                    sp_add_digits(cb, base + SP_A_LIMB, M, 0, iv < 0, mult);
                    // ahead of the group's first float (no float yet: the word is 0) the reference adds it as an int64, behind it as a
                    // double: v >> 32 of the former (nothing for [0, 2^32)), the wrapping sum of the latter (sp.cpp, package)
                    const unsigned long long ff = a.rows[mx + SP_M_FIRST_FLT];
                    if (~gidx > ff) { if (iv >> 32) cb.add(base + SP_A_PRE_HI, (unsigned long long) (iv >> 32) * mult); }
                    else cb.add(base + SP_A_POST_ISUM, (unsigned long long) iv * mult);
                }
            }
            else {
                cb.add(base + SP_A_NFLT, mult);
                if (~gidx > a.rows[mx + SP_M_FIRST_FLT]) atomicMax(&a.rows[mx + SP_M_FIRST_FLT], ~gidx);
                const uint64_t mag = v & ~nc::DBL_SIGN;
                if (mag > nc::DBL_INF_BITS) cb.add(base + SP_A_NAN, mult);
                else {
                    const unsigned long long o = sp_ord_f(v);
                    if (~o > a.rows[mx + 2]) atomicMax(&a.rows[mx + 2], ~o);
                    if (o > a.rows[mx + 3]) atomicMax(&a.rows[mx + 3], o);
                    if (mag == nc::DBL_INF_BITS) cb.add(base + ((v & nc::DBL_SIGN) ? SP_A_NINF : SP_A_PINF), mult);
                    else {
                        uint64_t M;
                        int64_t E;
                        nc::bits_to_me(mag, false, M, E);
                        sp_add_digits(cb, base + SP_A_LIMB, M, E, (v & nc::DBL_SIGN) != 0, mult);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < L2M_AGG_SLOTS; s += blockDim.x) {
        uint32_t key = keys[s];
        if (key && vals[s]) atomicAdd(&a.rows[key - 1], vals[s]);
    }
}

__global__ void k_sp_normalize(SpAggArgs a) {
    const uint32_t ng = *a.n_series;
    const uint64_t A = 1 + (uint64_t) SP_SRC_MAX * a.nsrc;
    const uint64_t total = (uint64_t) ng * a.nsrc;
    for (uint64_t q = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t g = q / a.nsrc, s = q % a.nsrc;
        unsigned long long *l = a.rows + g * a.W + A + 1 + SP_SRC_ADD * s + SP_A_LIMB;
        long long carry = 0;
        for (int j = 0; j < L2M_NLIMB - 1; j++) {
            long long t = (long long) l[j] + carry;
            long long lo = t & 0xFFFFFFFFll;
            carry = (t - lo) >> 32;
            l[j] = (unsigned long long) lo;
        }
        l[L2M_NLIMB - 1] = (unsigned long long) ((long long) l[L2M_NLIMB - 1] + carry);
    }
}

void launch_sp_extract(const SpArgs &a, int cus, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    const size_t lds = (size_t) (SP_BLOCK / 64) * SP_TILE;
    if (!attr_set) { (void) hipFuncSetAttribute((const void *) k_sp_extract, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); attr_set = true; }
    uint64_t want = (a.n + SP_BLOCK - 1) / SP_BLOCK;
    uint64_t grid = (uint64_t) cus * 2;
    if (grid > want) grid = want;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_sp_extract, dim3((unsigned) grid), dim3(SP_BLOCK), lds, st, a);
}
void launch_sp_generic(const SpArgs &a, hipStream_t st) {
    uint64_t grid = (a.n + 63) / 64;
    if (grid > 4096) grid = 4096;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_sp_generic, dim3((unsigned) grid), dim3(64), 0, st, a);
}
void launch_sp_aggregate(const SpAggArgs &a, int cus, bool first_float_pass, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    const size_t lds = (size_t) L2M_AGG_SLOTS * 12;
    if (!attr_set) { (void) hipFuncSetAttribute((const void *) k_sp_aggregate, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); attr_set = true; }
    uint64_t want = (a.n + L2M_AGG_BLOCK - 1) / L2M_AGG_BLOCK;
    uint64_t grid = (uint64_t) cus * 2;
    if (grid > want) grid = want;
    if (grid == 0) grid = 1;
    if (first_float_pass) hipLaunchKernelGGL(k_sp_first_float, dim3((unsigned) grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sp_aggregate, dim3((unsigned) grid), dim3(L2M_AGG_BLOCK), lds, st, a);
    hipLaunchKernelGGL(k_sp_normalize, dim3(64), dim3(256), 0, st, a);
}
