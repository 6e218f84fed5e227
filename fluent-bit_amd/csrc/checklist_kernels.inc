// checklist_kernels.inc -- filter_checklist (plugins/filter_checklist/checklist.c:291-409 set_record, 411-582 one call): a lane per
// record.  The size pass decodes the row, fetches the lookup value (ra_lds.inc), decides the match -- a probe of the open-addressed
// table in HBM (mode exact) or SQLite's LIKE over two buckets of the list (mode partial) --, keeps a flag byte per row and sizes the
// re-encoded record of a matched row.  The plan turns flags into output lengths once the host knows the first match that leaves
// something in the output; the emit pass writes every row into its own [out_off[r], out_off[r + 1]) and no further.  ONE function,
// cl_record, writes a record into a CountSink or a BoundedSink (canon_walk.inc), so both passes walk the same code.
// Every loop over list or record bytes is bounded by a length (never by a sentinel); every list offset is range-checked against
// the arena before it is read.  Included inside namespace flbgpu after kdev.inc, lane_rows.inc, canon_walk.inc and ra_lds.inc.

struct ClTable {
    const LDS_AS uint32_t *w;       // the table's words in LDS
    uint32_t nrec;
};

DEV uint32_t cl_fold(uint32_t c, int fold) { return (fold && c >= 'A' && c <= 'Z') ? c + 32u : c; }
DEV uint32_t cl_fold4(uint32_t x, int fold) {
    if (!fold) return x;
    uint32_t o = 0;
    for (int b = 0; b < 4; b++) o |= cl_fold((x >> (8 * b)) & 0xffu, 1) << (8 * b);
    return o;
}

// ---- mode exact: flb_hash_table_get's answer is membership, so the table is this project's own (checklist.hpp)
DEV bool cl_bytes_eq(const uint8_t *e, const uint8_t *v, uint32_t L, int fold) {
    uint32_t j = 0;
    bool eq = true;
    for (; eq && j + 4 <= L; j += 4) eq = ldu32(e + j) == cl_fold4(ldu32(v + j), fold);      // 4 bytes remain on both sides
    for (; eq && j < L; j++) eq = ld8(e + j) == cl_fold(ld8(v + j), fold);
    return eq;
}

DEV bool cl_exact(const ChecklistArgs &a, const uint8_t *v, uint32_t L) {
    if (L == 0 || a.nslots == 0) return false;                        // flb_hash_table_get refuses key_len <= 0
    uint64_t h = 0xcbf29ce484222325ull;
    uint32_t j = 0;
    for (; j + 4 <= L; j += 4) {
        const uint32_t x = cl_fold4(ldu32(v + j), a.fold);
        for (int b = 0; b < 4; b++) h = (h ^ ((x >> (8 * b)) & 0xffu)) * 0x100000001b3ull;
    }
    for (; j < L; j++) h = (h ^ cl_fold(ld8(v + j), a.fold)) * 0x100000001b3ull;
    const uint32_t mask = a.nslots - 1;
    uint32_t pos = (uint32_t) h & mask;
    for (uint32_t k = 0; k < a.nslots; k++) {                         // bounded by the slot count, whatever the table holds
        const v4u32 s = *(const v4u32 *) (a.slots + 4 * (size_t) pos);
        if (s.z == CL_EMPTY) return false;
        if (s.w == L && s.z <= a.arena_bytes && L <= a.arena_bytes - s.z && cl_bytes_eq(a.arena + s.z, v, L, a.fold)) return true;
        pos = (pos + 1) & mask;
    }
    return false;
}

// ---- mode partial: `value LIKE (entry || '%')`, case_sensitive_like on, as SQLite's patternCompare decides it
// the value: its bytes folded on the fly; past its length it reads as the terminator
struct ClStr {
    const uint8_t *p;
    uint32_t n;
    int fold;
    DEV uint32_t at(uint32_t i) const { return i < n ? cl_fold(ld8(p + i), fold) : 0u; }
};
// the pattern: the entry, one '%', the terminator
struct ClPat {
    const uint8_t *p;
    uint32_t n;
    DEV uint32_t at(uint32_t i) const { return i < n ? ld8(p + i) : (i == n ? (uint32_t) '%' : 0u); }
};

// SQLite's character reader: a lead byte >= 0xc0 takes every continuation byte behind it; overlong forms, surrogates and
// U+FFFE / U+FFFF read as U+FFFD; a stray continuation byte is a character of its own.  i ends behind the character.
template <class R> DEV uint32_t cl_u8read(const R &s, uint32_t &i) {
    uint32_t c = s.at(i);
    i++;
    if (c >= 0xc0u) {
        c = c < 0xe0u ? (c & 0x1fu) : c < 0xf0u ? (c & 0x0fu) : c < 0xf8u ? (c & 0x07u) : c < 0xfcu ? (c & 0x03u) : c < 0xfeu ? (c & 0x01u) : 0u;
        uint32_t b;
        while (((b = s.at(i)) & 0xc0u) == 0x80u) { c = (c << 6) + (b & 0x3fu); i++; }     // at() is 0 / '%' past the length: the loop ends there
        if (c < 0x80u || (c & 0xFFFFF800u) == 0xD800u || (c & 0xFFFFFFFEu) == 0xFFFEu) c = 0xFFFDu;
    }
    return c;
}

// the walker: no recursion, no stack, ONE restart point.  patternCompare's recursion never comes back to an outer '%' once an
// inner one was reached (its NOWILDCARDMATCH ends every level), so the innermost '%' is the only place a match is tried again.
// Behind a '%' the next pattern character c is searched in the value: as a raw byte when c <= 0x80 (strcspn in the original, so
// U+0080 is found inside other characters), as a character otherwise.  Every trip of the outer loop either consumes a pattern
// character or moves the restart point at least one byte forward.
DEV bool cl_like(const ClPat &pt, const ClStr &s) {
    uint32_t pi = 0, si = 0, r_pi = 0, r_si = 0, r_c = 0;
    bool have = false;
    for (;;) {
        uint32_t c = cl_u8read(pt, pi);
        if (c == 0) return s.at(si) == 0;
        if (c == '%') {
            for (;;) {                                                // a run of '%' and '_': each '_' takes one character
                c = cl_u8read(pt, pi);
                if (c == '%') continue;
                if (c == '_') { if (cl_u8read(s, si) == 0) return false; continue; }
                break;
            }
            if (c == 0) return true;                                  // the end of the entry: success
            r_c = c; r_pi = pi; r_si = si; have = true;
        }
        else {
            const uint32_t c2 = cl_u8read(s, si);
            if (c == c2) continue;
            if (c == '_' && c2 != 0) continue;
            if (!have) return false;
        }
        si = r_si;
        if (r_c <= 0x80u) {
            uint32_t b = 0;
            while (si < s.n && (b = s.at(si)) != 0 && b != r_c) si++;
            if (si >= s.n || b == 0) return false;
            si++;
        }
        else {
            for (;;) {
                const uint32_t c2 = cl_u8read(s, si);
                if (c2 == 0) return false;
                if (c2 == r_c) break;
            }
        }
        r_si = si;
        pi = r_pi;
    }
}

// the value's first byte chooses a literal bucket; the `any` bucket (entries that begin with '%', '_' or a byte >= 0x80) is walked too
DEV bool cl_partial(const ChecklistArgs &a, const uint8_t *v, uint32_t L) {
    const ClStr s{v, L, a.fold};
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 0 && L == 0) continue;
        const uint32_t bk = pass == 0 ? s.at(0) : 256u;
        uint32_t e = a.bucket_off[bk], hi = a.bucket_off[bk + 1];
        if (hi > a.nents) hi = a.nents;
        for (; e < hi; e++) {
            const uint32_t off = a.ents[2 * (size_t) e], len = a.ents[2 * (size_t) e + 1];
            if (off > a.arena_bytes || len > a.arena_bytes - off) continue;
            if (cl_like(ClPat{a.arena + off, len}, s)) return true;
        }
    }
    return false;
}

// ---- set_record (:291-409) into s; false: the row is not one well-formed event
template <class S> DEV bool cl_record(const ClTable &tb, const Event &ev, const uint8_t *end, S &s) {
    put_event_head(s, (uint32_t) ev.sec, (uint32_t) ev.nsec);
    put_meta(s, ev);
    uint8_t *hdr = open_map32(s);
    uint64_t kept = 0;
    const bool whole = put_entries(s, mp_tok(ev.body, end), end, [&](uint32_t, const uint8_t *e0, const uint8_t *) {
        const Tok k = mp_tok(e0, end);
        bool drop = k.type != T_STR;                                  // (:333-335)
        for (uint32_t ri = 0; !drop && ri < tb.nrec; ri++) {          // a key a `record` entry overrides (:338-360)
            const LDS_AS uint32_t *r = tb.w + CL_HDR_WORDS + CL_REC_WORDS * ri;
            drop = k.len == r[0] && lds_eq(tb.w + (r[1] >> 2), r[0], k.next);
        }
        if (drop) return ENTRY_DROP;
        kept++;
        return ENTRY_KEEP;
    });
    if (!whole) return false;
    for (uint32_t ri = 0; ri < tb.nrec; ri++) {                       // the `record` pairs in configuration order (:366-398)
        const LDS_AS uint32_t *r = tb.w + CL_HDR_WORDS + CL_REC_WORDS * ri;
        put_lds(s, tb.w + (r[3] >> 2), r[2]);
    }
    close_map32(s, hdr, kept + tb.nrec);
    return true;
}

constexpr uint8_t CLF_BAD = 0xff;

// size pass of one row: its flags (CLF_BAD: the decoder refuses it)
DEV uint8_t cl_size(const ChecklistArgs &a, const ClTable &tb, uint64_t r, uint64_t &enc_len, bool &nonstr) {
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    if (rec == end) return CLF_SKIP;                                  // a record an earlier filter dropped
    const Event ev = decode_event(rec, end, false);
    if ((ev.flags & RF_BAD) || ev.body_end != end) return CLF_BAD;
    if (ev.flags & RF_SKIP) return CLF_SKIP;                          // group markers: the decoder steps over them
    uint8_t fl = CLF_DECODED;
    const uint32_t acc = tb.w[1];
    bool match = false;
    if (!(acc & CL_ACC_INERT)) {
        // flb_ra_get_value_object (src/flb_record_accessor.c:803-814): a path may end on an array index
        const uint8_t *v = ra_lds_path(tb.w, tb.w + (tb.w[2] >> 2), acc & 0xffffu, tb.w + (tb.w[3] >> 2), (acc >> 16) & 0xffu, ev.body, end, true);
        if (v) {
            const Tok t = mp_tok(v, end);
            if (t.type == T_STR) match = a.mode == CL_EXACT ? cl_exact(a, t.next, t.len) : cl_partial(a, t.next, t.len);
            else nonstr = true;
        }
    }
    if (!match) return fl;
    fl |= CLF_MATCH;
    if (encoder_refuses_time(ev.sec, ev.nsec)) return fl;             // set_record's -2: rolled back, still a match (:549-555)
    CountSink cs;
    if (!cl_record(tb, ev, end, cs)) return CLF_BAD;
    enc_len = cs.n;
    return fl | CLF_OK;
}

// emit pass: a re-encoded record or the row's own bytes, into the row's room and no further; true: the lengths agree
DEV bool cl_emit(const ChecklistArgs &a, const ClTable &tb, uint64_t r) {
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    uint8_t *o0 = a.out + a.out_off[r], *o1 = a.out + a.out_off[r + 1];
    BoundedSink bs(o0, o1);
    const uint8_t fl = a.flags[r];
    if ((fl & CLF_MATCH) && r >= a.first_eff) {
        const Event ev = decode_event(rec, end, false);
        if (ev.flags & RF_BAD) return false;
        if (!cl_record(tb, ev, end, bs)) return false;
    }
    else put_span(bs, rec, (uint64_t) (end - rec));
    return !bs.over && bs.p == o1;
}

template <bool EMIT>
__global__ void __launch_bounds__(CL_BLOCK) k_checklist(ChecklistArgs a) {
    LDS_AS uint32_t *lds = lane_stage_table<CL_BLOCK>(a.table, a.table_bytes);
    __syncthreads();
    const ClTable tb{lds, lds[0]};
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long n_dec = 0, n_match = 0, n_rolled = 0, n_nonstr = 0, n_big = 0, n_mis = 0;
    // lane_wave_rows' loop, written out: through the helper's lambda the size pass measured 1 % slower over a long list, written out 1 %
    // faster than it was (DESIGN 4n).  Every wave walks in step (the trip count is the wave's, not the lane's): the ballots see whole waves.
    for (uint64_t r0 = (uint64_t) blockIdx.x * CL_BLOCK + (threadIdx.x & ~63u), gsz = (uint64_t) gridDim.x * CL_BLOCK; r0 < a.n; r0 += gsz) {
        const uint64_t r = r0 + (threadIdx.x & 63u);
        const bool live = r < a.n;
        if (EMIT) {
            if (live && a.len[r] && !cl_emit(a, tb, r)) n_mis++;
            continue;
        }
        uint8_t fl = 0;
        if (live) {
            uint64_t enc = 0;
            bool nonstr = false;
            fl = cl_size(a, tb, r, enc, nonstr);
            const uint64_t raw = a.row_off[r + 1] - a.row_off[r];
            if (fl == CLF_BAD) { atomicMin(&a.firsts[0], (unsigned long long) r); fl = 0; }
            else if (enc > 0xFFFFFFFFull || raw > 0xFFFFFFFFull) { n_big++; enc = 0; }   // a row the u32 length column cannot hold
            a.flags[r] = fl;
            a.enc_len[r] = (uint32_t) enc;
            if (nonstr && fl) n_nonstr++;
            if (fl & CLF_MATCH) { n_match++; if (!(fl & CLF_OK)) n_rolled++; }
        }
        const unsigned long long b_dec = lane_count(n_dec, (fl & CLF_DECODED) != 0), b_match = __ballot((fl & CLF_MATCH) != 0),
                                 b_ok = __ballot((fl & CLF_OK) != 0);
        if (lane == 0) {
            // the first rows of their kind (r is the wave's first row here): one atomic per wave and kind that has one
            if (b_dec) atomicMin(&a.firsts[1], (unsigned long long) (r + __ffsll((long long) b_dec) - 1));
            if (b_match) atomicMin(&a.firsts[2], (unsigned long long) (r + __ffsll((long long) b_match) - 1));
            if (b_ok) atomicMin(&a.firsts[3], (unsigned long long) (r + __ffsll((long long) b_ok) - 1));
        }
    }
    if (EMIT) { lane_flush(&a.counts[6], n_mis); return; }
    n_match = lane_wave_sum(n_match); n_rolled = lane_wave_sum(n_rolled); n_nonstr = lane_wave_sum(n_nonstr);
    lane_flush(&a.counts[0], n_dec);                                                                          // (lane 0's)
    if (lane == 0) { lane_flush(&a.counts[2], n_match); lane_flush(&a.counts[3], n_rolled); lane_flush(&a.counts[4], n_nonstr); }
    lane_flush(&a.counts[5], n_big);
}

// the first matched row behind a.after (the first record of the chunk matched and the encoder refused it)
__global__ void __launch_bounds__(CL_BLOCK) k_checklist_second(ChecklistArgs a) {
    const uint64_t gsz = (uint64_t) gridDim.x * CL_BLOCK;
    for (uint64_t r = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x; r < a.n; r += gsz)
        if (r > a.after && (a.flags[r] & CLF_MATCH)) atomicMin(&a.firsts[4], (unsigned long long) r);
}

// the plan (:537-563): F = a.first_eff.  In front of F everything up to the end of the last decoded row goes out as one raw span;
// F and every later matched row go out re-encoded when the encoder took them, else not at all; a later unmatched row goes out as
// its own bytes.  What the decoder stepped over travels with the next decoded row -- or is lost with it.
__global__ void __launch_bounds__(CL_BLOCK) k_checklist_plan(ChecklistArgs a) {
    const uint64_t gsz = (uint64_t) gridDim.x * CL_BLOCK;
    unsigned long long n_out = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * CL_BLOCK + threadIdx.x; r < a.n; r += gsz) {
        const uint8_t fl = a.flags[r];
        const uint32_t raw = (uint32_t) (a.row_off[r + 1] - a.row_off[r]);
        uint32_t len = 0;
        if (fl & CLF_DECODED) {
            if (r < a.first_eff || !(fl & CLF_MATCH)) len = raw;
            else if (fl & CLF_OK) len = a.enc_len[r];
            if (len) n_out++;
        }
        else {
            // a run of rows the decoder steps over is settled by its first row alone, for the whole run: every row is read once
            if (r > 0 && !(a.flags[r - 1] & CLF_DECODED)) continue;
            uint64_t q = r + 1;
            while (q < a.n && !(a.flags[q] & CLF_DECODED)) q++;       // bounded by the number of rows
            const bool keep = q < a.n && (q < a.first_eff || (q > a.first_eff && !(a.flags[q] & CLF_MATCH)));
            for (uint64_t k = r; k < q; k++) a.len[k] = keep ? (uint32_t) (a.row_off[k + 1] - a.row_off[k]) : 0u;
            continue;
        }
        a.len[r] = len;
    }
    if (n_out) atomicAdd(&a.counts[1], n_out);
}

void launch_checklist(const ChecklistArgs &a, bool emit, hipStream_t st) {
    if (a.n == 0) return;
    if (emit) hipLaunchKernelGGL(k_checklist<true>, dim3(lane_blocks<CL_BLOCK>(a.n)), dim3(CL_BLOCK), a.table_bytes, st, a);
    else hipLaunchKernelGGL(k_checklist<false>, dim3(lane_blocks<CL_BLOCK>(a.n)), dim3(CL_BLOCK), a.table_bytes, st, a);
}

void launch_checklist_second(const ChecklistArgs &a, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_checklist_second, dim3(lane_blocks<CL_BLOCK>(a.n)), dim3(CL_BLOCK), 0, st, a);
}

void launch_checklist_plan(const ChecklistArgs &a, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_checklist_plan, dim3(lane_blocks<CL_BLOCK>(a.n)), dim3(CL_BLOCK), 0, st, a);
}
