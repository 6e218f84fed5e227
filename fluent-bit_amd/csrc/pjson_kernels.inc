// pjson_kernels.inc -- filter_parser with a Format json parser: the size pass (included by kernels.hip).
// The emit pass is the regex path's (k_parser_emit / k_parser_emit_exact -> write_record).
//
//   k_pjson_size          one record per lane out of LDS tiles: decode the event, try every candidate value
//                         of Key_Name with flb_parser_json_do's rules (pjson_dev.inc), keep the last success
//                         (filter_parser.c:259-323), size the output record
//   k_pjson_size_generic  the records whose JSON is nested deeper than the register bit stack or holds a
//                         decimal that needs the exact conversion: same code with the wide stack and the
//                         big-integer path; they are emitted by k_parser_emit_exact

template <bool EXACT, int NW>
DEV uint32_t pjson_record(const ParserMatchArgs &a, uint64_t r, const uint8_t *rec, const uint8_t *rec_end, LDS_AS uint8_t *slot,
                          uint32_t &n_dec, bool &defer) {
    const DevParser &ps = a.parsers[0];
    RecInfo ri;
    recinfo_init(ri);
    defer = false;
    Event ev = decode_event(rec, rec_end);
    ri.flags = ev.flags;
    if (ev.flags & RF_BAD) { atomicMin(a.first_bad, (unsigned long long) r); rec_store(a.info, a.n, r, ri); a.null_mask[r] = 0; return 0; }
    if (ev.flags & RF_SKIP) { rec_store(a.info, a.n, r, ri); a.null_mask[r] = 0; return 0; }
    n_dec++;
    ri.body_off = (uint32_t) (ev.body - rec); ri.body_len = (uint32_t) (ev.body_end - ev.body);
    if (ev.meta) { ri.meta_off = (uint32_t) (ev.meta - rec); ri.meta_len = (uint32_t) (ev.meta_end - ev.meta); }
    uint64_t null_mask = 0;
    int64_t tsec = ev.sec, tnsec = ev.nsec;
    bool have_out = false, last_ok = false;
    uint32_t ntried = 0, win_bytes = 0;
    JsonCounts cc;
    cc.col = a.caps; cc.n = a.n; cc.r = r; cc.store = true;
    Tok bm = mp_tok(ev.body, ev.body_end);
    const uint8_t *p = bm.next;
    const uint32_t nkv = a.cfg.key.is_ra ? 1 : bm.len;
    for (uint32_t i = 0; i < nkv; i++) {
        const uint8_t *vptr = nullptr;
        uint32_t vlen = 0;
        if (a.cfg.key.is_ra) {
            const uint8_t *v = ra_resolve(a.cfg.key, ev.body, ev.body_end);
            if (v) {
                Tok t = mp_tok(v, ev.body_end);
                if (t.type == T_STR || t.type == T_BIN) { vptr = t.next; vlen = t.len; }
            }
        }
        else {
            Tok kt = mp_tok(p, ev.body_end);
            const uint8_t *kend = mp_end_of(kt, p, ev.body_end);
            Tok vt = mp_tok(kend, ev.body_end);
            p = mp_end_of(vt, kend, ev.body_end);
            if ((kt.type == T_STR || kt.type == T_BIN) && kt.len == (uint32_t) a.cfg.key.key_len &&
                bytes_eq(kt.next, a.cfg.key.key, kt.len) && (vt.type == T_STR || vt.type == T_BIN)) { vptr = vt.next; vlen = vt.len; }
        }
        if (!vptr) continue;
        cc.next = 0;
        PjsonTry t = ps.kv_format ? pkv_try(ps, vptr, vlen) : pjson_try<EXACT, NW>(ps, vptr, vlen, cc, slot);
        ntried++;
        if (t.defer || t.need_exact) {
            if constexpr (!EXACT) { defer = true; return 0; }          // (with the wide stack: deeper than 4096 levels = unparsable)
        }
        // several parsers: the next one of the list gets the value this one refused (filter_parser.c:259-300);
        // k_parser_generic runs the whole list
        if constexpr (!EXACT) { if (!t.ok && a.cfg.nparsers > 1) { defer = true; return 0; } }
        last_ok = t.ok;
        if (t.ok) {
            have_out = true;
            ri.val_off = (uint32_t) (vptr - rec); ri.val_len = vlen; ri.parser_idx = 0; ri.nkept = t.npairs; ri.drop_mask = t.skip;
            win_bytes = t.bytes;
            if (!a.cfg.key.is_ra) {
                ri.key_index = i;
                null_note(a.cfg, r, i, null_mask);
            }
            if ((uint64_t) t.sec * 1000000000ull + (uint64_t) t.nsec != 0) { tsec = t.sec; tnsec = t.nsec; }
        }
    }
    if (have_out && last_ok) {
        ri.flags |= RF_PARSED;
        if (ntried > 1 && !ps.kv_format) {
            // a later candidate overwrote the container-count columns: put the winner's back
            cc.next = 0;
            (void) pjson_try<EXACT, NW>(ps, rec + ri.val_off, ri.val_len, cc, slot);
        }
    }
    a.null_mask[r] = null_mask;
    // encoder timestamp check (src/flb_log_event_encoder.c:345-363)
    if (encoder_refuses_time(tsec, tnsec)) {
        ri.flags |= RF_BADTS;
        rec_store(a.info, a.n, r, ri);
        return 0;
    }
    ri.ts_sec = (uint32_t) tsec; ri.ts_nsec = (uint32_t) tnsec;
    if ((ri.flags & RF_PARSED) && (uint32_t) tsec >= 0xfffffffeu) atomicAdd(&a.counts[MW_TIME_MARKER], 1ull);     // (a group marker to the next decoder: tile_kernels.inc k_parser_reg)
    CapsView caps;
    caps.base = a.caps; caps.n = a.n; caps.r = r;
    CountSink cs;
    if ((ri.flags & RF_PARSED) && !a.cfg.reserve_data && !(a.cfg.preserve_key && !a.cfg.key.is_ra)) {
        // nothing is appended: header + metadata + map header + the pairs sized by the walk above
        cs.n = 12;
        if (ri.meta_len > 1) mp_canon(rec + ri.meta_off, rec + ri.meta_off + ri.meta_len, cs); else cs.n += 1;
        pk_map_hdr(cs, ri.nkept);
        cs.n += win_bytes;
    }
    else write_record<EXACT, NW>(cs, a.cfg, a.parsers, rec, rec_end, ri, caps, null_mask);
    rec_store(a.info, a.n, r, ri);
    return (uint32_t) cs.n;
}

constexpr int PJ_BLOCK = 256;
constexpr int PJ_TILE = 14336;              // LDS bytes per wave for the records ...
constexpr int PJ_SLOTS = 64 * 64;           // ... plus a 64-byte slot per lane for a decoded time string

__global__ void __launch_bounds__(PJ_BLOCK) k_pjson_size(ParserMatchArgs a) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LDS_AS uint8_t *tile = (LDS_AS uint8_t *) g_lds + (size_t) wave * (PJ_TILE + PJ_SLOTS);
    LDS_AS uint8_t *slot = tile + PJ_TILE + lane * 64;
    const uint64_t wave_id = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    const uint8_t *data_end = a.data + a.bytes;
    uint32_t n_dec = 0, n_gen = 0;
    for (uint64_t base = wave_id * 64; base < a.n; base += nwaves * 64) {
        const uint64_t r = base + lane;
        const uint32_t cnt = (uint32_t) ((a.n - base) < 64 ? (a.n - base) : 64);
        uint64_t o0 = 0, o1 = 0;
        if (lane < cnt) { o0 = a.row_off[r]; o1 = a.row_off[r + 1]; }
        uint32_t lo = 0;
        while (lo < cnt) {
            const uint64_t g0 = __shfl(o0, (int) lo, 64);
            const uint32_t align = (uint32_t) (g0 & 15);
            const bool fit = lane >= lo && lane < cnt && (o1 - g0 + align) <= (uint64_t) PJ_TILE;
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
                const uint8_t *rec, *rec_end;
                if (direct) { rec = a.data + o0; rec_end = a.data + o1; }
                else { rec = (const uint8_t *) (tile + align + (uint32_t) (o0 - g0)); rec_end = rec + (o1 - o0); }
                bool defer = false;
                const uint32_t ol = pjson_record<false, 1>(a, r, rec, rec_end, slot, n_dec, defer);
                // (the single-parser generic kernel counts the record again; k_parser_generic does not)
                if (defer) { a.info[r] = RF_VALID | RF_GENERIC; a.out_len[r] = 0; n_gen++; if (a.cfg.nparsers <= 1) n_dec--; }
                else a.out_len[r] = ol;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            lo += m;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { n_dec += __shfl_down(n_dec, o, 64); n_gen += __shfl_down(n_gen, o, 64); }
    if (lane == 0) {
        if (n_dec) atomicAdd(&a.counts[MW_DECODED], (unsigned long long) n_dec);
        if (n_gen) atomicAdd(&a.counts[MW_GENERIC], (unsigned long long) n_gen);
    }
}

__global__ void __launch_bounds__(64) k_pjson_size_generic(ParserMatchArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t slots[64 * 64];
    LDS_AS uint8_t *slot = (LDS_AS uint8_t *) slots + threadIdx.x * 64;
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (uint64_t) gridDim.x * blockDim.x) {
        if (!(a.info[r] & RF_GENERIC)) continue;
        uint32_t n_dec = 0;
        bool defer = false;
        uint32_t ol = pjson_record<true, JSON_GENERIC_WORDS>(a, r, a.data + a.row_off[r], a.data + a.row_off[r + 1], slot, n_dec, defer);
        // (defer can only mean "deeper than 4096 levels" here: the value is treated as unparsable)
        a.out_len[r] = ol;
        if (ol) { a.info[r] |= RF_EXACT; atomicAdd(&a.counts[MW_EXACT], 1ull); }
        if (n_dec) atomicAdd(&a.counts[MW_DECODED], (unsigned long long) n_dec);
    }
}

void launch_pjson_size(const ParserMatchArgs &a, int cus, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    const size_t lds = (size_t) (PJ_BLOCK / 64) * (PJ_TILE + PJ_SLOTS);
    if (!attr_set) { (void) hipFuncSetAttribute((const void *) k_pjson_size, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); attr_set = true; }
    uint64_t want = (a.n + PJ_BLOCK - 1) / PJ_BLOCK;
    uint64_t grid = (uint64_t) cus * 2;
    if (grid > want) grid = want;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_pjson_size, dim3((unsigned) grid), dim3(PJ_BLOCK), lds, st, a);
}
void launch_pjson_size_generic(const ParserMatchArgs &a, hipStream_t st) {
    uint64_t grid = (a.n + 63) / 64;
    if (grid > 4096) grid = 4096;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_pjson_size_generic, dim3((unsigned) grid), dim3(64), 0, st, a);
}
