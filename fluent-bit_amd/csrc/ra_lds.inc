// ra_lds.inc -- the record accessor's key lookup against a rule table that sits in LDS (typeconv_kernels.inc, rtag_kernels.inc): the
// last-key-wins search of ra_key_val_id and the sub-key walk of subkey_to_object (src/flb_ra_key.c:108-135, 151-236).  A sub-key
// list is two words per sub-key: { index | RA_LDS_SUB_INDEX, 0 } or { length, byte offset of the name inside the table }.
// Included inside namespace flbgpu after kdev.inc.

constexpr uint32_t RA_LDS_SUB_INDEX = 0x80000000u;

// are the L bytes at key (all of them inside the record: mp_tok checked the payload) the entry at e?  A 4-byte load is issued
// only where 4 bytes remain inside the key.
DEV bool lds_eq(const LDS_AS uint32_t *e, uint32_t L, const uint8_t *key) {
    uint32_t j = 0;
    bool eq = true;
    for (; eq && j + 4 <= L; j += 4) eq = ldu32(key + j) == e[j >> 2];
    for (; eq && j < L; j++) eq = ld8(key + j) == ((e[j >> 2] >> (8 * (j & 3))) & 0xffu);
    return eq;
}

// ra_key_val_id (src/flb_ra_key.c:108-135): the value of the LAST entry of the map at `map` whose key is a STR equal to the name
DEV const uint8_t *ra_lds_find_last(const uint8_t *map, const uint8_t *end, const LDS_AS uint32_t *name, uint32_t nlen) {
    Tok m = mp_tok(map, end);
    if (m.type != T_MAP) return nullptr;
    const uint8_t *p = m.next, *found = nullptr;
    for (uint32_t i = 0; i < m.len; i++) {
        Tok k = mp_tok(p, end);
        const uint8_t *v = mp_end_of(k, p, end, 2);
        if (!v) return nullptr;
        if (k.type == T_STR && k.len == nlen && lds_eq(name, nlen, k.next)) found = v;
        p = mp_end_of(mp_tok(v, end), v, end, 2);
        if (!p) return nullptr;
    }
    return found;
}

// the top-level entry `name`, then the sub-keys when its value is a map or an array (any other value is taken as it is:
// flb_ra_key_to_value_ext :250-271, flb_ra_key_regex_match :391-413).  tbl: the table's words; index_ok: a path that ends on an
// array index is a value (subkey_to_object answers it with no key object, which only flb_ra_get_kv_pair's callers refuse).
DEV const uint8_t *ra_lds_path(const LDS_AS uint32_t *tbl, const LDS_AS uint32_t *name, uint32_t nlen, const LDS_AS uint32_t *sub, uint32_t nsub,
                               const uint8_t *body, const uint8_t *end, bool index_ok) {
    const uint8_t *val = ra_lds_find_last(body, end, name, nlen);
    if (!val) return nullptr;
    Tok t = mp_tok(val, end);
    if ((t.type != T_MAP && t.type != T_ARRAY) || nsub == 0) return val;
    const uint8_t *cur = val;
    uint32_t matched = 0;
    bool last_index = false;
    for (uint32_t s = 0; s < nsub; s++) {
        Tok c = mp_tok(cur, end);
        const uint32_t s0 = sub[2 * s];
        if (s0 & RA_LDS_SUB_INDEX) {
            const uint32_t idx = s0 & ~RA_LDS_SUB_INDEX;
            if (c.type != T_ARRAY || idx >= c.len) return nullptr;
            const uint8_t *p = c.next;
            for (uint32_t i = 0; i < idx; i++) { p = mp_skip(p, end); if (!p) return nullptr; }
            cur = p;
            last_index = true;
            if (++matched == nsub) break;
            continue;
        }
        if (c.type != T_MAP) break;
        const uint8_t *v = ra_lds_find_last(cur, end, tbl + (sub[2 * s + 1] >> 2), s0);
        if (!v) continue;                          // "try next entry": the levels are never completed
        cur = v;
        last_index = false;
        if (++matched == nsub) break;
    }
    if (matched != nsub || (last_index && !index_ok)) return nullptr;
    return cur;
}
