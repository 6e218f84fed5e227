// expect_kernels.inc -- filter_expect (plugins/filter_expect/expect.c:275-396 rule_apply, 398-564 one call): a lane per record, the
// rule table in LDS.  k_expect<EX_CHECK> decodes the row, runs the rules in order up to the first one that fails and keeps a verdict
// word per row (with the span of the STR value the rule met); k_expect<EX_SIZE> does the same and sizes the rebuilt record --
// {result_key: bool} in front of the body's own entries -- into a CountSink; k_expect<EX_EMIT> writes every row into its own
// [out_off[r], out_off[r + 1]) through the bounded sink and no further.  ONE function, ex_record, writes a record into either sink,
// so both passes walk the same code.  k_expect_table places one entry per failing row in record order from a scan over the fail flags.
// Every loop is bounded by a length (never by a sentinel); nothing recurses.  Included inside namespace flbgpu after kdev.inc,
// lane_rows.inc, canon_walk.inc and ra_lds.inc.

struct ExTable {
    const LDS_AS uint32_t *w;       // the table's words in LDS
    uint32_t nrules;
};

// msgpack_object_to_ra_value (src/flb_ra_key.c:31-105): a MAP reads as a boolean, a BIN as a binary, an ARRAY or EXT is no value
DEV uint32_t ex_vtype(int t) {
    switch (t) {
    case T_BOOL: case T_MAP: return EXT_BOOL;
    case T_UINT: case T_NINT: return EXT_INT;
    case T_F32: case T_F64: return EXT_FLOAT;
    case T_STR: return EXT_STRING;
    case T_BIN: return EXT_BINARY;
    case T_NIL: return EXT_NULL;
    default: return EXT_NONE;
    }
}

// rule_apply (:275-396): 0 when every rule passes, else the verdict of the first rule that fails.  voff / vlen: the payload of the
// STR value that rule met, relative to rec.
DEV uint32_t ex_rules(const ExTable &tb, const uint8_t *rec, const uint8_t *body, const uint8_t *end, uint32_t &voff, uint32_t &vlen) {
    for (uint32_t ri = 0; ri < tb.nrules; ri++) {
        const LDS_AS uint32_t *r = tb.w + EX_HDR_WORDS + EX_RULE_WORDS * ri;
        const uint32_t kind = r[0], acc = r[1];
        if (kind == EX_ACTION) continue;                                // (its value is fetched and never looked at)
        uint32_t vt = EXT_NONE;
        Tok t;
        t.type = T_BAD; t.len = 0; t.u = 0; t.next = nullptr;
        if (!(acc & EX_ACC_INERT)) {
            // flb_ra_get_value_object (src/flb_record_accessor.c:803-814): a path may end on an array index
            const uint8_t *v = ra_lds_path(tb.w, tb.w + (r[2] >> 2), acc & 0xffffu, tb.w + (r[3] >> 2), (acc >> 16) & 0xffu, body, end, true);
            if (v) { t = mp_tok(v, end); vt = ex_vtype(t.type); }
        }
        uint32_t how = 0;
        switch (kind) {
        case EX_KEY_EXISTS: if (vt == EXT_NONE) how = EXF_NOT_FOUND; break;
        case EX_KEY_NOT_EXISTS: if (vt != EXT_NONE) how = EXF_EXISTS; break;
        case EX_KEY_VAL_NULL: how = vt == EXT_NONE ? EXF_NOT_FOUND : vt != EXT_NULL ? EXF_WRONG_TYPE : 0; break;
        case EX_KEY_VAL_NOT_NULL: how = vt == EXT_NONE ? EXF_NOT_FOUND : vt == EXT_NULL ? EXF_WRONG_TYPE : 0; break;
        default:
            // flb_sds_cmp: the lengths, then strncmp over them -- the expected text is a C string, so no NUL ends the walk early
            if (vt == EXT_NONE) how = EXF_NOT_FOUND;
            else if (vt == EXT_STRING && (t.len != r[4] || !lds_eq(tb.w + (r[5] >> 2), r[4], t.next))) how = EXF_DIFFERENT;
            break;
        }
        if (!how) continue;
        if (vt == EXT_STRING) { voff = (uint32_t) (t.next - rec); vlen = t.len; }
        return EXV_FAILED | ri | (how << 8) | (vt << 12);
    }
    return 0;
}

// the rebuilt record (:498-532) into s: EventTime, the metadata re-packed, a map32 header for the body's entries and one more, the
// result entry, the body's entries re-packed.  false: the row is not one well-formed event
template <class S> DEV bool ex_record(const ExTable &tb, const Event &ev, const uint8_t *end, bool failed, S &s) {
    put_event_head(s, (uint32_t) ev.sec, (uint32_t) ev.nsec);
    put_meta(s, ev);
    const Tok bm = mp_tok(ev.body, end);
    s.put(0xdf);
    pk_be(s, (uint64_t) bm.len + 1, 4);
    put_lds(s, tb.w + (tb.w[3] >> 2), tb.w[2]);
    s.put(failed ? 0xc2 : 0xc3);
    return put_entries(s, bm, end, [](uint32_t, const uint8_t *, const uint8_t *) { return ENTRY_KEEP; });
}

struct ExRow {
    bool bad;               // the decoder refuses the row
    uint32_t verdict, voff, vlen;
    uint64_t len;           // size pass: output bytes
};

// check / size pass of one row
template <int PASS> DEV ExRow ex_row(const ExpectArgs &a, const ExTable &tb, uint64_t r) {
    ExRow w;
    w.bad = false; w.verdict = 0; w.voff = 0; w.vlen = 0; w.len = 0;
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    if (rec == end) return w;                                           // a record an earlier filter dropped
    const Event ev = decode_event(rec, end, false);
    if ((ev.flags & RF_BAD) || ev.body_end != end) { w.bad = true; return w; }
    if (ev.flags & RF_SKIP) {
        // -1 s and -2 s are the group markers: raw under result_key (:486-496), unseen otherwise; any other negative time the
        // decoder itself steps over (src/flb_log_event_decoder.c:397-414)
        if (ev.sec == -1 || ev.sec == -2) { w.verdict = EXV_RAW; if (PASS == EX_SIZE) w.len = (uint64_t) (end - rec); }
        return w;
    }
    w.verdict = EXV_CHECKED | ex_rules(tb, rec, ev.body, end, w.voff, w.vlen);
    if (PASS == EX_SIZE && !encoder_refuses_time(ev.sec, ev.nsec)) {
        // (a time the EventTime cannot hold: set_timestamp's answer is overwritten by the next decoder call and the record is gone)
        CountSink cs;
        if (!ex_record(tb, ev, end, (w.verdict & EXV_FAILED) != 0, cs)) { w.bad = true; return w; }
        w.len = cs.n;
    }
    return w;
}

// emit pass: the rebuilt record or the marker's own bytes, into the row's room and no further; true: the lengths agree
DEV bool ex_emit(const ExpectArgs &a, const ExTable &tb, uint64_t r) {
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    uint8_t *o0 = a.out + a.out_off[r], *o1 = a.out + a.out_off[r + 1];
    BoundedSink bs(o0, o1);
    const uint32_t vd = a.verdict[r];
    if (vd & EXV_RAW) put_span(bs, rec, (uint64_t) (end - rec));
    else {
        const Event ev = decode_event(rec, end, false);
        if (ev.flags & RF_BAD) return false;
        if (!ex_record(tb, ev, end, (vd & EXV_FAILED) != 0, bs)) return false;
    }
    return !bs.over && bs.p == o1;
}

// Three waves a SIMD, not the five the register count would allow: every lane streams its own record, and the fewer waves share a
// CU's cache the more of each record's lines are still there when its lane comes back for them (DESIGN 4l has the measurement:
// the check pass with four rules 6.98 ms at five waves, 3.91 ms at four, 2.57 ms at three).  -DEX_WAVES=n builds another bound.
#ifndef EX_WAVES
#define EX_WAVES 3
#endif
template <int PASS>
__global__ void __attribute__((amdgpu_waves_per_eu(EX_WAVES, EX_WAVES))) __launch_bounds__(EX_BLOCK) k_expect(ExpectArgs a) {
    LDS_AS uint32_t *lds = lane_stage_table<EX_BLOCK>(a.table, a.table_bytes);
    __syncthreads();
    const ExTable tb{lds, lds[0]};
    unsigned long long n_chk = 0, n_fail = 0, n_out = 0, n_big = 0, n_mis = 0;
    lane_wave_rows<EX_BLOCK>(a.n, [&](uint64_t r, bool live) {
        if (PASS == EX_EMIT) {
            if (live && a.len[r] && !ex_emit(a, tb, r)) n_mis++;
            return;
        }
        ExRow w;
        w.bad = false; w.verdict = 0; w.voff = 0; w.vlen = 0; w.len = 0;
        if (live) {
            w = ex_row<PASS>(a, tb, r);
            const uint64_t raw = a.row_off[r + 1] - a.row_off[r];
            if (w.bad) { atomicMin(&a.firsts[0], (unsigned long long) r); w.verdict = 0; w.len = 0; }
            else if (w.len > 0xFFFFFFFFull || raw > 0xFFFFFFFFull) { n_big++; w.len = 0; }      // a row the u32 columns cannot hold
            a.verdict[r] = w.verdict;
            a.val_off[r] = w.voff;
            a.val_len[r] = w.vlen;
            a.fail[r] = (w.verdict & EXV_FAILED) ? 1u : 0u;
            if (PASS == EX_SIZE) a.len[r] = (uint32_t) w.len;
        }
        lane_count(n_chk, (w.verdict & EXV_CHECKED) != 0);
        lane_count(n_out, w.len != 0 && (w.verdict & EXV_CHECKED) != 0);                                    // (records, not markers)
        const unsigned long long b_fail = lane_count(n_fail, (w.verdict & EXV_FAILED) != 0);
        // the first failing row (r is the wave's first row on lane 0): one atomic per wave that has one
        if ((threadIdx.x & 63u) == 0 && b_fail) atomicMin(&a.firsts[1], (unsigned long long) (r + __ffsll((long long) b_fail) - 1));
    });
    if (PASS == EX_EMIT) { lane_flush(&a.counts[4], n_mis); return; }
    lane_flush(&a.counts[0], n_chk); lane_flush(&a.counts[1], n_fail); lane_flush(&a.counts[2], n_out);      // (lane 0's: one atomic a wave)
    lane_flush(&a.counts[3], n_big);
}

// the failure table: the entry of failing row r stands at fail_idx[r], so the table is in record order whatever the launch order was
__global__ void __launch_bounds__(EX_BLOCK) k_expect_table(ExpectArgs a) {
    const uint64_t gsz = (uint64_t) gridDim.x * EX_BLOCK;
    for (uint64_t r = (uint64_t) blockIdx.x * EX_BLOCK + threadIdx.x; r < a.n; r += gsz) {
        const uint32_t vd = a.verdict[r];
        if (!(vd & EXV_FAILED)) continue;
        const uint64_t at = a.fail_idx[r];
        if (at >= a.fail_cap) continue;
        ExFailure e;
        e.in_off = a.row_off[r];
        e.len = (uint32_t) (a.row_off[r + 1] - a.row_off[r]);
        e.rule = vd & 0xffu; e.kind = (vd >> 8) & 0xfu; e.vtype = (vd >> 12) & 0xfu; e.reserved = 0;
        e.val_off = e.vtype == EXT_STRING ? a.row_off[r] + a.val_off[r] : 0;       // (no span for a value that is no STR)
        e.val_len = a.val_len[r];
        a.fail_tbl[at] = e;
    }
}

void launch_expect(const ExpectArgs &a, int pass, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 g(lane_blocks<EX_BLOCK>(a.n)), b(EX_BLOCK);
    if (pass == EX_EMIT) hipLaunchKernelGGL(k_expect<EX_EMIT>, g, b, a.table_bytes, st, a);
    else if (pass == EX_SIZE) hipLaunchKernelGGL(k_expect<EX_SIZE>, g, b, a.table_bytes, st, a);
    else hipLaunchKernelGGL(k_expect<EX_CHECK>, g, b, a.table_bytes, st, a);
}

void launch_expect_table(const ExpectArgs &a, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_expect_table, dim3(lane_blocks<EX_BLOCK>(a.n)), dim3(EX_BLOCK), 0, st, a);
}
