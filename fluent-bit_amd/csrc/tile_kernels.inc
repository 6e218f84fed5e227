// tile_kernels.inc -- filter_parser's pass 1 in ONE pass over the chunk (k_parser_tile).
//
// The phase kernels (k_parser_locate / k_parser_rx / k_parser_finish) read the chunk three times -- twice through
// per-lane 64-byte windows that touch every cache line two or three times -- and hand spans, time text and record
// fields to each other through HBM columns.  Here a wave copies its 64 records (one contiguous range of the chunk)
// into LDS once with coalesced 16 B / lane loads, and every lane then takes its record all the way:
//
//   locate   decode the event, find the value Key_Name designates           (locate_core, from the tile)
//   walk     parser 0's capture program, forward from boundary 0             (compact tables DevFx, dev.hpp)
//   finish   named fields, fixed-layout time lookup, size of the parsed record
//   rules    pair mode: filter_grep's rules on the spans                      (plugins/filter_grep/grep.c:167-194,250-284)
//
// and writes columns only for the rows something downstream reads: every row's flags / size / keep_len, the full
// record columns and spans only for rows that are emitted later or that a general kernel has to finish (the time
// text needs the strptime interpreter, several candidate keys, bytes >= 0x80, Types / Reserve_Data sizes, ...).
//
// The walk: one dword of value bytes per four steps from the tile (aligned ds_read_b32 + v_alignbit), byte -> class*4
// through a 256-byte table, entry = ft[row + class] with every offset in bytes, ONE unconditional capture write
// (column 0 is a dummy), and nothing else on the plain path.  The end of the text is a byte: 0xFF, written behind the
// value in the tile, is the end-of-text column; what MATCH / dead ends / multi-candidate cells were in the classic
// tables are plain steps into an absorbing row whose capture write records the position, so the loop has no exits
// and the only non-plain entries are the one-byte look-ahead and the (rare) double capture write.
// Patterns: start-anchored ones (DevParser::fwd_first) whose compact tables fit (DevFx::ok).  A value the forward
// walk does not match goes through the reverse pass + classic forward walk (tables in global memory: rare).

#include <utility>

constexpr uint32_t FX_CAP_STRIDE = 128;          // bytes between capture columns of a wave ([slot][lane] u16)

DEV uint32_t fx_special(uint32_t e, uint32_t cn, LDS_AS const uint8_t *lds, uint32_t p2_at, LDS_AS uint8_t *capcol, uint32_t j) {
    if (!(e & 0x40000000u)) {
        // the next byte decides (one-byte look-ahead)
        e = *(LDS_AS const uint32_t *) (lds + ((e & FX_ROW_MASK) + cn));
        if ((int32_t) e >= 0) return e;
    }
    // two capture writes: the second one here, the first with the plain entry
    LDS_AS const uint32_t *p2 = (LDS_AS const uint32_t *) (lds + p2_at) + 2 * (e & 0x3FFFFFFFu);
    *(LDS_AS uint16_t *) (capcol + p2[1]) = (uint16_t) j;
    return p2[0];
}

// (the same for a lane that is known to hold one; tables at LDS address 0)
DEV uint32_t fx_pair_do(uint32_t e, uint32_t p2_at, LDS_AS uint8_t *capcol, uint32_t j) {
    LDS_AS const uint32_t *p2 = (LDS_AS const uint32_t *) (uintptr_t) (p2_at + 8 * (e & 0x3FFFFFFFu));
    *(LDS_AS uint16_t *) (capcol + p2[1]) = (uint16_t) j;
    return p2[0];
}
// the (rare) entry with two capture writes, for the lanes that hold one: the second write here, the first with the plain entry
DEV uint32_t fx_pair(uint32_t e, LDS_AS const uint8_t *lds, uint32_t p2_at, LDS_AS uint8_t *capcol, uint32_t j) {
    if ((int32_t) e < 0) {
        LDS_AS const uint32_t *p2 = (LDS_AS const uint32_t *) (lds + p2_at) + 2 * (e & 0x3FFFFFFFu);
        *(LDS_AS uint16_t *) (capcol + p2[1]) = (uint16_t) j;
        e = p2[0];
    }
    return e;
}

// forward walk of one value in the tile; vaddr = LDS byte address of the value, ngroups uniform; the tables sit at LDS
// address 0 (cls: 256 dwords, then the rows: dev.hpp DevFx).  Returns the final row.
DEV uint32_t fx_walk(LDS_AS const uint8_t *lds, const DevFx &fx, uint32_t vaddr, uint32_t ngroups, LDS_AS uint8_t *capcol) {
    LDS_AS const uint32_t *clsT = (LDS_AS const uint32_t *) lds;
    LDS_AS const uint32_t *vw = (LDS_AS const uint32_t *) (lds + (vaddr & ~3u));
    const uint32_t sh = (vaddr & 3u) * 8, p2_at = fx.off_p2;
    uint32_t e = fx.start_off, j = 0;
    uint32_t dlo = vw[0], dhi = vw[1];
    uint32_t w = __builtin_amdgcn_alignbit(dhi, dlo, sh);
    uint32_t c0 = clsT[w & 255], c1 = clsT[(w >> 8) & 255], c2 = clsT[(w >> 16) & 255], c3 = clsT[w >> 24];
#define FX_STEP(ck, cn)                                                                      \
    {                                                                                        \
        e = *(LDS_AS const uint32_t *) (lds + ((e & FX_ROW_MASK) + (ck)));                   \
        if (__builtin_expect((int32_t) e < 0, 0)) e = fx_special(e, (cn), lds, p2_at, capcol, j); \
        *(LDS_AS uint16_t *) (capcol + (e >> FX_SLOT_SHIFT)) = (uint16_t) j;                 \
        j++;                                                                                 \
    }
    #pragma unroll 1
    for (uint32_t g = 0; g < ngroups; g++) {
        // bytes and classes of the next group, one trip ahead of their use
        dlo = dhi; dhi = vw[g + 2];
        const uint32_t wn = __builtin_amdgcn_alignbit(dhi, dlo, sh);
        const uint32_t n0 = clsT[wn & 255], n1 = clsT[(wn >> 8) & 255], n2 = clsT[(wn >> 16) & 255], n3 = clsT[wn >> 24];
        FX_STEP(c0, c1) FX_STEP(c1, c2) FX_STEP(c2, c3) FX_STEP(c3, n0)
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
#undef FX_STEP
    return e & FX_ROW_MASK;
}

// the rare way: reverse pass + classic forward walk on the value in global memory (tables in global memory too).
// >= 0: end of the match (spans in the capture columns), -1 no match, -2 a byte >= 0x80 (UTF-8 tables: generic kernel)
__device__ __noinline__ int tile_capture_slow(const DevParser *ps, const uint8_t *val, uint32_t vlen, uint16_t *chk, LDS_AS uint8_t *capcol, uint32_t cap_step = FX_CAP_STRIDE) {
    HotTabs<false> h = hot_global(ps->ascii);
    const int best = rx_reverse(h, ps->ascii.r_info, val, vlen, chk);
    if (best < 0) return best;
    CapLds c;
    c.base = capcol; c.stride_b = cap_step;
    for (int i = 0; i < 2 * ps->nfields; i++) c.set((uint32_t) i, CAP_UNSET);
    return rx_forward(ps->ascii, h, val, vlen, best, chk, ps->slot2cap, c);
}

struct TileCaps {
    CapLds c;
    DEV uint32_t operator[](uint32_t i) const { return c.get(i); }
};

__global__ void __launch_bounds__(512) k_parser_tile(ParserMatchArgs a) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LDS_AS uint8_t *lds = (LDS_AS uint8_t *) g_lds;
    const DevParser &ps = a.parsers[0];
    const DevFx fx = ps.fx;
    {
        // compact tables and (pair mode) the rules' match-only DFAs: one copy per workgroup
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        const v4u *src = (const v4u *) fx.base;
        LDS_AS v4u *dst = (LDS_AS v4u *) g_lds;
        for (uint32_t i = threadIdx.x; i < fx.bytes / 16; i += blockDim.x) dst[i] = src[i];
        if (a.pg) {
            LDS_AS uint8_t *pg_lds = lds + a.pg_lds_off;
            for (int i = 0; i < a.pg->nrules; i++) {
                if (a.pg->rule_lds_off[i] == 0xFFFFFFFFu) continue;
                const uint8_t *rs = a.pg->rules[i].dfa.cls;
                for (uint32_t k = threadIdx.x; k < a.pg->rule_lds_bytes[i]; k += blockDim.x) pg_lds[a.pg->rule_lds_off[i] + k] = rs[k];
            }
        }
        __syncthreads();
    }
    const uint32_t tile_off = a.tile_lds_off + wave * a.tile_wave_bytes;
    LDS_AS uint8_t *tile = lds + tile_off;
    LDS_AS uint8_t *capcol = tile + TILE_BYTES + 2 * lane;
    CapLds capl;
    capl.base = capcol; capl.stride_b = FX_CAP_STRIDE;
    const uint32_t wave_slot = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    uint16_t *chk = a.chk + ((size_t) wave_slot * a.chk_len) * 64 + lane;
    const uint8_t *data_end = a.data + a.bytes;
    const int ncap = 2 * ps.nfields;
    const bool size_from_columns = !a.cfg.reserve_data && !(a.cfg.preserve_key && !a.cfg.key.is_ra) && ps.plain_types;
    const uint64_t n = a.n;
    uint32_t n_dec = 0, n_gen = 0, n_fin = 0, n_slow = 0, pg_out = 0, pg_keep = 0, pg_pending = 0;
    unsigned long long pg_bytes = 0;
    for (uint64_t base = (uint64_t) wave_slot * 64; base < n; base += nwaves * 64) {
        const uint64_t r = base + lane;
        const uint32_t cnt = (uint32_t) ((n - base) < 64 ? (n - base) : 64);
        uint64_t o0 = 0, o1 = 0;
        if (lane < cnt) { o0 = a.row_off[r]; o1 = a.row_off[r + 1]; }
        uint32_t lo = 0;
        while (lo < cnt) {
            // ---- the records lo .. lo+m-1 of this group that fit the tile together (normally all of them)
            const uint64_t g0 = __shfl(o0, (int) lo, 64);
            const uint32_t align = (uint32_t) (g0 & 15);
            const bool fit = lane >= lo && lane < cnt && (o1 - g0 + align) < (uint64_t) TILE_BYTES;     // (< : room for the sentinel)
            const uint64_t mask = __ballot(fit) >> lo;
            uint32_t m = (~mask == 0) ? 64 - lo : (uint32_t) __builtin_ctzll(~mask);
            if (m > cnt - lo) m = cnt - lo;
            const bool direct = (m == 0);                 // one record larger than the tile: located in place, walked by the generic kernel
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
            const bool act = lane >= lo && lane < lo + m;
            RecInfo ri;
            recinfo_init(ri);
            uint32_t out_len = 0, rec_lds = 0;
            const uint8_t *recg = a.data + o0;
            if (act) {
                const uint8_t *rec, *rec_end;
                if (direct) { rec = recg; rec_end = a.data + o1; }
                else { rec_lds = align + (uint32_t) (o0 - g0); rec = (const uint8_t *) (tile + rec_lds); rec_end = rec + (o1 - o0); }
                out_len = locate_core(a, r, rec, rec_end, n_dec, ri);
                if (direct && (ri.flags & RF_CAND)) { ri.flags = (ri.flags & ~(uint32_t) RF_CAND) | RF_GENERIC; atomicAdd(&a.counts[MW_GENERIC], 1ull); }
            }
            const bool cand = act && (ri.flags & RF_CAND);
            const uint32_t vlen = ri.val_len;
            // every lane has read its header: the sentinels may overwrite the first byte of the next record
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            if (cand) {
                tile[rec_lds + ri.val_off + vlen] = 0xFF;
                for (uint32_t c = 0; c < fx.nslots; c++) *(LDS_AS uint16_t *) (capcol + c * FX_CAP_STRIDE) = 0xFFFF;
            }
            uint32_t maxlen = cand ? vlen : 0;
            for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t) __shfl_xor((int) maxlen, o, 64); maxlen = t > maxlen ? t : maxlen; }
            maxlen = (uint32_t) __builtin_amdgcn_readfirstlane((int) maxlen);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            int endb = -1;                                  // >= 0 match end, -1 no match, -2 bytes >= 0x80
            if (cand) {
                const uint32_t S = fx_walk(lds, fx, tile_off + rec_lds + ri.val_off, maxlen / 4 + 1, capcol);
                const uint32_t e_eot = capl.get((uint32_t) ncap + FXS_END_EOT - 1), e_mid = capl.get((uint32_t) ncap + FXS_END_MID - 1),
                               d_eot = capl.get((uint32_t) ncap + FXS_DEAD_EOT - 1), failed = capl.get((uint32_t) ncap + FXS_FAIL - 1);
                int res;                                    // 1 match, 0 no match at boundary 0 / undecided, -2 poison
                if (S == fx.poison_off) res = -2;
                else if (failed != CAP_UNSET) res = 0;
                else if (e_mid != CAP_UNSET) { res = 1; endb = (int) e_mid; }
                else if (e_eot != CAP_UNSET) { if (e_eot == vlen) { res = 1; endb = (int) vlen; } else res = -2; }
                else if (d_eot != CAP_UNSET) res = d_eot == vlen ? 0 : -2;
                else res = 0;
                if (res == -2) endb = -2;
                else if (res == 0) { n_slow++; endb = tile_capture_slow(&ps, recg + ri.val_off, vlen, chk, capcol); }   // a later start (line anchors), or none
            }
            if (act) {
                uint32_t flags = ri.flags;
                bool done = false;                           // the row is complete: parsed, sized, (pair mode) decided
                bool caps_valid = false, will_finish = false;
                uint32_t keep_len = PG_UNDECIDED;
                uint64_t null_mask = 0;
                if (cand && endb >= 0) {
                    flags |= RF_RXOK;
                    caps_valid = true;
                    // ---- named fields, time, size (k_parser_finish's fast path); pair mode: the rules (k_parser_rx's block)
                    bool any = false, slow = !size_from_columns;
                    uint32_t kept = 0, drop = 0, body_bytes = 0, pgdrop = a.pg ? a.pg->static_drop : 0;
                    int64_t sec = 0;
                    for (int f = 0; f < ps.nfields; f++) {
                        const uint32_t b = capl.get((uint32_t) (2 * f)), e = capl.get((uint32_t) (2 * f + 1));
                        const bool set = b != CAP_UNSET && e != CAP_UNSET;
                        any |= set;
                        const uint32_t fl = set ? e - b : 0;
                        if (fl == 0 && ps.skip_empty) { drop |= 1u << f; pgdrop |= 1u << f; continue; }
                        if (ps.field_is_time[f]) {
                            int64_t s2;
                            if (f == ps.time_field && ps.plan.ok && fl == (uint32_t) ps.plan.len &&
                                time_fast(ps, (LDS_AS const uint8_t *) (tile + rec_lds + ri.val_off + b), &s2)) sec = s2;
                            else { slow = true; continue; }
                            if (!ps.time_keep) { drop |= 1u << f; continue; }
                        }
                        kept++;
                        const uint32_t nl = (uint32_t) ps.field_name_len[f];
                        body_bytes += (nl < 32 ? 1 : nl < 256 ? 2 : nl < 65536 ? 3 : 5) + nl + (fl < 32 ? 1 : fl < 256 ? 2 : fl < 65536 ? 3 : 5) + fl;
                    }
                    uint32_t pgbits = 0;
                    if (a.pg && any) {
                        uint32_t named = 0;
                        for (int i = 0; i < a.pg->nrules; i++) named |= a.pg->rule_fmask[i];
                        if (!(named & a.pg->time_fields & ~pgdrop)) {
                            TileCaps cv{capl};
                            const bool keep = pg_grep_parsed<true>(a.pg->rules, a.pg->nrules, a.pg->logical_op, a.pg->rule_fmask, a.pg->rule_lds_off, pgdrop,
                                                             recg + ri.val_off, cv, (LDS_AS const uint8_t *) (lds + a.pg_lds_off));
                            pgbits = RF_PGDONE | (keep ? RF_PGKEEP : 0u);
                        }
                    }
                    flags |= pgbits;
                    if (!any) {
                        // flb_regex_parse found no participating named group: the parser fails (k_parser_finish)
                        if (a.cfg.nparsers > 1) { flags |= RF_GENERIC; n_gen++; }
                    }
                    else if (slow) {
                        // k_parser_finish takes over: it reads the spans and the time text from the columns
                        n_fin++;
                        will_finish = true;
                        if (ps.time_field >= 0) {
                            const uint32_t tb = capl.get((uint32_t) (2 * ps.time_field)), te = capl.get((uint32_t) (2 * ps.time_field + 1));
                            if (tb != CAP_UNSET && te != CAP_UNSET && te - tb <= 4 * TBUF_WORDS) {
                                const uint32_t tl = te - tb;
                                const uint8_t *tv = recg + ri.val_off + tb;
                                v4u32 w0 = load16(tv, 0, tl), w1 = load16(tv + 16, 0, tl > 16 ? tl - 16 : 0);
                                a.tbuf[0 * n + r] = w0.x; a.tbuf[1 * n + r] = w0.y; a.tbuf[2 * n + r] = w0.z; a.tbuf[3 * n + r] = w0.w;
                                a.tbuf[4 * n + r] = w1.x; a.tbuf[5 * n + r] = w1.y; a.tbuf[6 * n + r] = w1.z; a.tbuf[7 * n + r] = w1.w;
                            }
                        }
                    }
                    else {
                        done = true;
                        if (!a.cfg.key.is_ra) null_note(a.cfg, r, ri.key_index, null_mask);
                        int64_t tsec = ri.ts_sec, tnsec = ri.ts_nsec;
                        if (flags & RF_BADTS) { tsec = -3; tnsec = 0; }                     // the event time was out of range
                        if (sec != 0) { tsec = sec; tnsec = 0; }                            // (the fixed-layout formats carry no fraction)
                        flags = (flags | RF_PARSED) & ~(uint32_t) RF_BADTS;
                        ri.parser_idx = 0; ri.nkept = kept; ri.drop_mask = drop;
                        // encoder timestamp check (src/flb_log_event_encoder.c:345-363)
                        if (encoder_refuses_time(tsec, tnsec)) {
                            flags |= RF_BADTS;
                            out_len = 0;
                            keep_len = 0;
                        }
                        else {
                            ri.ts_sec = (uint32_t) tsec; ri.ts_nsec = (uint32_t) tnsec;
                            if ((uint32_t) tsec >= 0xfffffffeu) atomicAdd(&a.counts[MW_TIME_MARKER], 1ull);     // (k_parser_reg: the next filter's decoder reads a group marker)
                            const uint32_t n0 = (uint32_t) ps.nregs_minus1;
                            out_len = 12 + ri.meta_canon + (n0 < 16 ? 1 : n0 < 65536 ? 3 : 5) + body_bytes;
                            if (a.pg_keep_len) {
                                if (pgbits & RF_PGDONE) {
                                    const bool keep = (pgbits & RF_PGKEEP) != 0;
                                    keep_len = keep ? out_len : 0;
                                    pg_out++; pg_bytes += out_len; pg_keep += keep ? 1u : 0u;
                                }
                                else pg_pending++;
                            }
                        }
                    }
                }
                else if (cand && (endb == -2 || a.cfg.nparsers > 1)) {
                    // a byte >= 0x80 (UTF-8 tables) or more parsers to try: the generic kernel takes over
                    flags |= RF_GENERIC;
                    n_gen++;
                }
                ri.flags = flags;
                // ---- columns: what a later kernel reads of this row
                if (!done) {
                    // k_parser_finish's treatment of a row it does not parse; a row it will finish itself (will_finish) is left alone
                    if (!will_finish) {
                        if (!(flags & RF_GENERIC)) a.null_mask[r] = 0;
                        if (a.pg_keep_len) { a.pg_keep_len[r] = PG_UNDECIDED; pg_pending++; }
                    }
                    rec_store(a.info, n, r, ri);
                    a.out_len[r] = out_len;
                    if (caps_valid) for (int c = 0; c < ncap; c++) a.caps[(uint64_t) c * n + r] = capl.get((uint32_t) c);
                }
                else {
                    const bool dropped = a.pg_keep_len && keep_len == 0;      // pair mode, settled, not kept: nothing reads the rest
                    if (a.pg_keep_len) a.pg_keep_len[r] = keep_len;
                    if (dropped) a.info[r] = flags;
                    else {
                        rec_store(a.info, n, r, ri);
                        a.null_mask[r] = null_mask;
                        a.out_len[r] = out_len;
                        for (int c = 0; c < ncap; c++) a.caps[(uint64_t) c * n + r] = capl.get((uint32_t) c);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            lo += m;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_dec += __shfl_down(n_dec, o, 64); n_gen += __shfl_down(n_gen, o, 64); n_fin += __shfl_down(n_fin, o, 64); n_slow += __shfl_down(n_slow, o, 64);
        pg_out += __shfl_down(pg_out, o, 64); pg_keep += __shfl_down(pg_keep, o, 64); pg_pending += __shfl_down(pg_pending, o, 64);
        pg_bytes += __shfl_down(pg_bytes, o, 64);
    }
    if (lane == 0) {
        if (n_dec) atomicAdd(&a.counts[MW_DECODED], (unsigned long long) n_dec);
        if (n_gen) atomicAdd(&a.counts[MW_GENERIC], (unsigned long long) n_gen);
        if (n_fin) atomicAdd(&a.counts[MW_FINISH], (unsigned long long) n_fin);
        if (n_slow) atomicAdd(&a.counts[MW_SLOW], (unsigned long long) n_slow);
        if (pg_bytes) atomicAdd(&a.counts[MW_PG_BYTES], pg_bytes);
        if (pg_keep) atomicAdd(&a.counts[MW_PG_KEEP], (unsigned long long) pg_keep);
        if (pg_out) atomicAdd(&a.counts[MW_PG_OUT], (unsigned long long) pg_out);
        if (pg_pending) atomicAdd(&a.counts[MW_PG_PENDING], (unsigned long long) pg_pending);
    }
}

// ------------------------------------------------------------------------------------------------------------------
#ifndef REG_STREAM
#define REG_STREAM 0          // 1: k_parser_reg keeps two 64-byte windows of the value in registers instead of all of it (see the kernel)
#endif
// k_parser_reg -- the same single pass with the value bytes in REGISTERS instead of an LDS tile.
//
// k_parser_tile is bound by the LDS: a wave's 64 records take 18 KB, seven waves fit a CU, and a wave's walk is a chain
// of dependent LDS reads (~200 cycles a byte), so the CU sits idle most of the time.  Here nothing of the record lives in
// the LDS: every lane reads the first 48 bytes of its record (header, key, value header of the layout every input plugin
// produces for a line of text: 92 92 d7 00 <ts> 80 81 <fixstr key> <str value>) and decodes them in registers -- any other
// layout goes through locate_core on the bytes in global memory --, then loads its value with one burst of 16-byte loads
// (all lanes of the wave together: each cache line of the chunk is requested in one short burst by the lanes that share
// it) into 17 x 4 registers.  The walk runs in lockstep over all lanes, so the byte position is uniform and the
// registers are addressed statically; values longer than 272 bytes continue through 64-byte windows loaded from memory.
// The end of the text is the 0xFF sentinel again, or-ed into the group that holds position `len`.  16 waves per CU.
// ------------------------------------------------------------------------------------------------------------------
constexpr int REG_THREADS = 1024;
// The fast pass is built twice: TB = 768 threads per workgroup (12 waves per CU, 168 registers a lane: NOTHING spilled -- the default)
// and TB = 1024 (16 waves, 128 registers, 60 of them in scratch: FLBGPU_TILE_WAVES=16).  Measured round 4: 1.92 against 1.96 ms per 10 M
// records -- four more waves buy what the scratch traffic costs (FETCH 4.7 GB / WRITE 0.70 GB per launch with the spills).
constexpr uint32_t REG_TSLOT = 4 * TBUF_WORDS + 4;      // per-lane LDS slot of the time text (+4: spreads the banks)

// 16 bytes at p, zeros from the end of the chunk on (the last loads of the last records reach past it)
__device__ __noinline__ v4u32 ld16_tail(const uint8_t *p, const uint8_t *data_end) {
    v4u32 v;
    uint32_t t4[4] = {0, 0, 0, 0};
    for (int q = 0; q < 16 && p + q < data_end; q++) t4[q >> 2] |= (uint32_t) ld8(p + q) << (8 * (q & 3));
    v.x = t4[0]; v.y = t4[1]; v.z = t4[2]; v.w = t4[3];
    return v;
}
DEV v4u32 ld16_guard(const uint8_t *p, const uint8_t *data_end) {
    if (__builtin_expect(p + 16 <= data_end, 1)) return ldu128(p);
    return ld16_tail(p, data_end);
}

// The value sits in registers (q: 17 x 16 bytes, addressed statically).  What the steps behind the walk need of it -- the
// time field's text, the few bytes a rule tests -- starts at a position every lane knows only now, so the bytes are taken
// out with a barrel shifter of selects: dwords d0 .. d0 + L - 1 (d0 <= 63) in 6 levels of v_cndmask, ~6 L + 57 operations
// and no memory access (the loads from the chunk this replaces were two dependent round trips to the L2 or further per
// record, for lines the wave had fetched 60 microseconds earlier).
// (pack expansions, not loops: every index is a constant from the start, so the temporaries never exist as arrays in memory)
template <int I> DEV uint32_t reg_qw(const v4u32 (&q)[18]) {
    if constexpr (I >= 68) return 0u;
    else if constexpr ((I & 3) == 0) return q[I >> 2].x;
    else if constexpr ((I & 3) == 1) return q[I >> 2].y;
    else if constexpr ((I & 3) == 2) return q[I >> 2].z;
    else return q[I >> 2].w;
}
template <int N> struct RegArr { uint32_t v[N]; };
template <int N, int... Is>
DEV RegArr<N> reg_sel_q(const v4u32 (&q)[18], bool b, std::integer_sequence<int, Is...>) { return RegArr<N>{{(b ? reg_qw<Is + 32>(q) : reg_qw<Is>(q))...}}; }
template <int N, int SH, int... Is>
DEV RegArr<N> reg_sel(const RegArr<N + SH> &in, bool b, std::integer_sequence<int, Is...>) { return RegArr<N>{{(b ? in.v[Is + SH] : in.v[Is])...}}; }
template <int L>
DEV void reg_extract(const v4u32 (&q)[18], uint32_t d0, uint32_t (&out)[L]) {
    const RegArr<L + 31> a32 = reg_sel_q<L + 31>(q, (d0 & 32) != 0, std::make_integer_sequence<int, L + 31>{});
    const RegArr<L + 15> a16 = reg_sel<L + 15, 16>(a32, (d0 & 16) != 0, std::make_integer_sequence<int, L + 15>{});
    const RegArr<L + 7> a8 = reg_sel<L + 7, 8>(a16, (d0 & 8) != 0, std::make_integer_sequence<int, L + 7>{});
    const RegArr<L + 3> a4 = reg_sel<L + 3, 4>(a8, (d0 & 4) != 0, std::make_integer_sequence<int, L + 3>{});
    const RegArr<L + 1> a2 = reg_sel<L + 1, 2>(a4, (d0 & 2) != 0, std::make_integer_sequence<int, L + 1>{});
    const RegArr<L> a1 = reg_sel<L, 1>(a2, (d0 & 1) != 0, std::make_integer_sequence<int, L>{});
    #pragma unroll
    for (int i = 0; i < L; i++) out[i] = a1.v[i];
}
// N dwords of text from byte position pos of the value in q (pos + 4 N <= 272)
template <int N>
DEV void reg_text(const v4u32 (&q)[18], uint32_t pos, uint32_t (&w)[N]) {
    uint32_t t[N + 1];
    reg_extract<N + 1>(q, pos >> 2, t);
    const uint32_t sh = (pos & 3) * 8;
    #pragma unroll
    for (int i = 0; i < N; i++) w[i] = __builtin_amdgcn_alignbit(t[i + 1], t[i], sh);
}
// the dword at byte position pos of the value's FIRST 64 bytes (pos <= 59): four levels of selects over q[0..4] instead of six over all of q
// (19 selects + the funnel shift; the year's digits of the time text, which sits behind a host and two short fields)
template <int N, int... Is>
DEV RegArr<N> reg_first(const v4u32 (&q)[18], std::integer_sequence<int, Is...>) { return RegArr<N>{{reg_qw<Is>(q)...}}; }
DEV uint32_t reg_dword_head(const v4u32 (&q)[18], uint32_t pos) {
    const uint32_t d0 = pos >> 2;
    const RegArr<17> all = reg_first<17>(q, std::make_integer_sequence<int, 17>{});
    const RegArr<9> a8 = reg_sel<9, 8>(all, (d0 & 8) != 0, std::make_integer_sequence<int, 9>{});
    const RegArr<5> a4 = reg_sel<5, 4>(a8, (d0 & 4) != 0, std::make_integer_sequence<int, 5>{});
    const RegArr<3> a2 = reg_sel<3, 2>(a4, (d0 & 2) != 0, std::make_integer_sequence<int, 3>{});
    const RegArr<2> a1 = reg_sel<2, 1>(a2, (d0 & 1) != 0, std::make_integer_sequence<int, 2>{});
    return __builtin_amdgcn_alignbit(a1.v[1], a1.v[0], (pos & 3) * 8);
}
// the time text as 8 registers; the plan's offsets are uniform (kernel arguments): a byte is a scalar branch and a shift
struct RegTimeText {
    uint32_t w[8];
    DEV uint32_t operator[](uint32_t o) const {
        const uint32_t u = (uint32_t) __builtin_amdgcn_readfirstlane((int) o);
        uint32_t d;
        switch (u >> 2) {
        case 0: d = w[0]; break; case 1: d = w[1]; break; case 2: d = w[2]; break; case 3: d = w[3]; break;
        case 4: d = w[4]; break; case 5: d = w[5]; break; case 6: d = w[6]; break; default: d = w[7]; break;
        }
        return (d >> (8 * (u & 3))) & 255u;
    }
};

// filter_grep's rules on the spans, from the compact rule table in the kernel arguments (TileCfg): the rule's match-only DFA
// sits in the LDS, a field of up to 16 bytes (status codes, methods, ...) comes in with one load; anything else -- a longer
// field, bytes >= 0x80 -- goes through the general pg_rule_match
// (round 5, measured and not kept: the first rule's 16 bytes requested right behind the walk and used behind the time phase -- 1.838 against
// 1.833 ms, the load's round trip is not what the iteration waits for)
// (UNGUARDED: the fast register kernel, whose loads never need a test -- a record near the end of the chunk is read from the padded
// copy of the chunk's tail --: the field comes in with ONE 16-byte load whatever its length; a guarded load of a 3-byte status code was
// three byte loads and four rounds of bounds logic)
// the 16 bytes at the start of named field `f` (span begin b), taken out of the value's registers by the caller; f < 0: not taken
struct RuleText { int f; uint32_t b; v4u32 w; };
template <bool UNGUARDED = false, class CV>
DEV int tc_rule_match(const TileRule &ru, const GrepRule *grules, int i, uint32_t drop, const uint8_t *val, const CV &caps, LDS_AS const uint8_t *pg_lds,
                      const RuleText rt = RuleText{-1, 0, (v4u32) (0)}) {
    const uint32_t m = ru.fmask & ~drop;
    if (!m) return -1;                                    // the key is not in the parsed record
    const uint32_t f = 31u - (uint32_t) __builtin_clz(m);
    const uint32_t b = caps[2 * f], e = caps[2 * f + 1];
    const bool set = b != CAP_UNSET && e != CAP_UNSET;
    const uint32_t len = set ? e - b : 0;
    if (len <= 16) {
        v4u32 w;
        if (UNGUARDED && rt.f == (int) f && set && rt.b == b) w = rt.w;
        else w = UNGUARDED ? ldu128(set ? val + b : val) : load16(set ? val + b : val, 0, len);
        LDS_AS const uint8_t *blk = pg_lds + ru.lds_off;
        const int r = pg_dfa_short(blk, (LDS_AS const uint16_t *) (blk + ru.o_dd), blk + ru.o_df, ru.ncls, ru.d_init, w, len);
        if (r != RX_POISON) return r == RX_MATCH ? 1 : 0;
    }
    // (kept inline: moved out of line -- it is 24 000 of the kernel's 35 000 instructions -- the calls' spills cost more than the
    // smaller kernel gained, 2.35 -> 2.63 ms; the instruction cache misses nothing either way: SQC_ICACHE_MISSES 0)
    return pg_rule_match<true>(grules[i], ru.fmask, drop, val, caps, pg_lds + ru.lds_off);
}
template <bool UNGUARDED = false, class CV>
DEV bool tc_grep_parsed(const TileCfg &tc, const GrepRule *grules, uint32_t drop, const uint8_t *val, const CV &caps, LDS_AS const uint8_t *pg_lds,
                        const RuleText rt = RuleText{-1, 0, (v4u32) (0)}) {
    bool keep = true;
    if (tc.pg_logical_op == OP_LEGACY) {
        // plugins/filter_grep/grep.c:167-194
        for (int i = 0; i < tc.pg_nrules; i++) {
            const int ret = tc_rule_match<UNGUARDED>(tc.rule[i], grules, i, drop, val, caps, pg_lds, i == 0 ? rt : RuleText{-1, 0, (v4u32) (0)});
            if (ret <= 0) { if (tc.rule[i].type == GREP_REGEX) { keep = false; break; } }
            else { keep = (tc.rule[i].type != GREP_EXCLUDE); break; }
        }
    }
    else {
        // plugins/filter_grep/grep.c:250-284
        bool found = false;
        int last = 0;
        for (int i = 0; i < tc.pg_nrules; i++) {
            last = i;
            found = tc_rule_match<UNGUARDED>(tc.rule[i], grules, i, drop, val, caps, pg_lds, i == 0 ? rt : RuleText{-1, 0, (v4u32) (0)}) > 0;
            if (tc.pg_logical_op == OP_OR && found) break;
            if (tc.pg_logical_op == OP_AND && !found) break;
        }
        if (tc.pg_nrules > 0) keep = (tc.rule[last].type == GREP_REGEX) ? found : !found;
    }
    return keep;
}

// Kill bytes (>= 0x80, or one of up to three byte values: dev.hpp DevFx::kill) among the positions [from, vlen) of the value in q: the
// dwords from `from / 4` (uniform) on, four bytes per test; bytes from vlen on are masked out (the sentinel and what follows it).
template <int D>
DEV void reg_kill_scan(const v4u32 (&q)[18], uint32_t d0, uint32_t d1, uint32_t vlen, uint32_t nkill, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t &bad) {
    if constexpr (D < 68) {
        if ((uint32_t) D >= d0 && (uint32_t) D <= d1) {                   // uniform
            const int nv = (int) vlen - 4 * D;
            const uint32_t m = nv >= 4 ? 0xFFFFFFFFu : nv <= 0 ? 0u : (0xFFFFFFFFu >> (32 - 8 * nv));
            const uint32_t w = reg_qw<D>(q) & m;
            uint32_t t = w & 0x80808080u;
            if (nkill > 0) { const uint32_t x = w ^ k0; t |= (x - 0x01010101u) & ~x & 0x80808080u; }
            if (nkill > 1) { const uint32_t x = w ^ k1; t |= (x - 0x01010101u) & ~x & 0x80808080u; }
            if (nkill > 2) { const uint32_t x = w ^ k2; t |= (x - 0x01010101u) & ~x & 0x80808080u; }
            // (a masked-out byte is 0x00: a kill byte 0x00 -- or a zero byte below a real hit -- reports too much, never too little)
            bad |= t & m;
        }
        reg_kill_scan<D + 1>(q, d0, d1, vlen, nkill, k0, k1, k2, bad);
    }
}

// A wave's maximum / minimum of a u32 without the LDS: four row shifts and the two row broadcasts of the GFX9 DPP (lane 63 ends up with
// the result).  (__shfl_xor is ds_bpermute_b32: six DEPENDENT trips through the LDS pipeline per reduction, each behind whatever the other
// waves of the CU have queued there -- three reductions per iteration were 18 of them, and six registers of permute addresses.)
DEV uint32_t wave_umax(uint32_t v) {
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false));
    return (uint32_t) __builtin_amdgcn_readlane((int) v, 63);
}
DEV uint32_t wave_umin(uint32_t v) { return ~wave_umax(~v); }

// byte i (compile-time constant after unrolling) of the 48 header bytes
#define REG_HB(i) ((hw[(i) >> 2] >> (8 * ((i) & 3))) & 255u)

// The two layouts input plugins produce for a line of text, decoded from the first 48 bytes of the record (hw):
//   MAP32 = false   92 92 d7 00 <sec> <nsec> 80 81 <fixstr key> <str value>            (set_*_from_msgpack_object: in_lib, in_dummy, ...)
//   MAP32 = true    92 92 d7 00 <sec> <nsec> df 00 00 00 00 df 00 00 00 01 <fixstr key> <str value>
//                   (begin_record + append_body_values: in_tail -- src/flb_mp.c:591-640 always reserves 32-bit map headers)
// Fills ri / out_len like locate_core and returns true; false: another layout (or a marker, a bad timestamp, trailing bytes):
// the general walk decides.
template <bool MAP32>
DEV bool reg_fast_decode(const uint32_t (&hw)[12], uint32_t klen, const char *key, uint32_t rlen, uint32_t caps_in_lds, uint32_t chk_len,
                         unsigned long long *counts, RecInfo &ri, uint32_t &out_len) {
    constexpr uint32_t KH = MAP32 ? 22 : 14;            // where the key's fixstr header sits
    bool ok = hw[0] == 0x00d79292u && REG_HB(KH) == (0xa0u | klen);
    if constexpr (MAP32) ok = ok && hw[3] == 0x000000dfu && hw[4] == 0x0000df00u && (hw[5] & 0xFFFFu) == 0x0100u;   // df 00 00 00 00 | df 00 00 00 01
    else ok = ok && REG_HB(12) == 0x80 && REG_HB(13) == 0x81;
    #pragma unroll
    for (uint32_t i = 0; i < 15; i++) if (i < klen) ok = ok && REG_HB(KH + 1 + i) == (uint32_t) (uint8_t) key[i];
    // the value header starts at byte KH + 1 + klen (uniform): five bytes from there
    uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0;
    #pragma unroll
    for (uint32_t k = 1; k <= 15; k++) if (k == klen) { v0 = REG_HB(KH + 1 + k); v1 = REG_HB(KH + 2 + k); v2 = REG_HB(KH + 3 + k); v3 = REG_HB(KH + 4 + k); v4 = REG_HB(KH + 5 + k); }
    uint32_t hdr = 0, vl = 0;
    if (v0 >= 0xa0 && v0 <= 0xbf) { hdr = 1; vl = v0 & 31; }
    else if (v0 == 0xd9) { hdr = 2; vl = v1; }
    else if (v0 == 0xda) { hdr = 3; vl = (v1 << 8) | v2; }
    else if (v0 == 0xdb) { hdr = 5; vl = (v1 << 24) | (v2 << 16) | (v3 << 8) | v4; }
    else ok = false;
    const uint32_t sec = __builtin_bswap32(hw[1]), nsec = __builtin_bswap32(hw[2]);
    const uint32_t voff = KH + 1 + klen + hdr;
    if (!(ok && sec < 0xfffffffeu && nsec < 1000000000u && (uint64_t) voff + vl == (uint64_t) rlen)) return false;
    ri.flags = RF_VALID;
    ri.meta_off = 12; ri.meta_len = MAP32 ? 5 : 1; ri.meta_canon = 1;                   // (an empty map re-packs as 80 either way)
    ri.body_off = MAP32 ? 17 : 13; ri.body_len = rlen - ri.body_off;
    ri.val_off = voff; ri.val_len = vl; ri.key_index = 0; ri.ts_sec = sec; ri.ts_nsec = nsec;
    if (caps_in_lds && vl < 0xFFFF && (vl / CHK_STEP + 2) <= chk_len) ri.flags |= RF_CAND;
    else { ri.flags |= RF_GENERIC; atomicAdd(&counts[MW_GENERIC], 1ull); }
    // the record if no parser matches: 92 92 d7 00 ts(8) 80 | 81 key value, canonical headers
    out_len = 12 + 1 + 1 + (1 + klen) + (vl < 32 ? 1 : vl < 256 ? 2 : vl < 65536 ? 3 : 5) + vl;
    return true;
}

// 16 bytes at any LDS byte address (ds_read_b128; the LDS takes unaligned addresses)
DEV v4u32 lds_ldu128(LDS_AS const uint8_t *p) {
    typedef v4u32 v4u32u __attribute__((aligned(1)));
    return *(LDS_AS const v4u32u *) p;
}

// SLOW = false: the kernel proper -- no calls in it (a call makes the register allocator spill what is live across it where it
// is DEFINED: 190 bytes of scratch stores per record showed up as 1.9 GB of WRITE_SIZE), every load in bounds without a test.
// A record it does not take -- another layout, or within 400 bytes of the end of the chunk, where a wide load could run past
// it -- is only flagged (RF_NEEDLOC); SLOW = true is the same code for exactly those rows, with the general locate_core,
// guarded loads and the reverse-pass fallback, launched when there are any.
// the general locate out of line, for the fix-up launch (inlined it sets the register budget of the whole kernel: the walk of
// k_parser_reg<true, ..> ran with 219 spilled registers).  ap: the DEVICE copy of the arguments (ParserMatchArgs::self) -- a pointer to
// the kernel's own argument block would pin all of it in scratch memory
__device__ __noinline__ uint32_t locate_core_ool(const ParserMatchArgs *ap, uint64_t r, const uint8_t *rec, const uint8_t *rec_end, uint32_t *n_dec, RecInfo *ri) {
    uint32_t nd = *n_dec;
    RecInfo t = *ri;
    const uint32_t ol = locate_core(*ap, r, rec, rec_end, nd, t);
    *n_dec = nd; *ri = t;
    return ol;
}

template <bool SLOW, bool STAGE = false, int FXK = 0, int TB = REG_THREADS>
// (REG_WAVES_PER_EU: experiment builds that force a smaller register budget -- 5 or 6 waves per SIMD with two workgroups per CU,
// FLBGPU_TILE_GRID_MULT=2 --; measured in round 4: 198 / 423 spills inside the walk, 3.4 ms against 2.2)
#ifdef REG_WAVES_PER_EU
__global__ void __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(REG_WAVES_PER_EU, REG_WAVES_PER_EU))) k_parser_reg(ParserMatchArgs a) {
#else
__global__ void __launch_bounds__(TB) k_parser_reg(ParserMatchArgs a) {
#endif
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LDS_AS uint8_t *lds = (LDS_AS uint8_t *) g_lds;
    const DevParser &ps = a.parsers[0];
    // FXK: which form of the compact tables the walk steps through -- 0: look-ahead / pair entries (fx.cpp build_fx), 3: no special
    // entries, 8-byte cells, one position per read (build_fx3), 4: the same cells composed in pairs, two positions per read
    // 5: the pairs with THREE capture-write ports (positions j - 1, j, j + 1; fx.cpp build_fx3 pairs = 2)
    constexpr bool FX3 = FXK >= 3, FX4 = FXK >= 4, FX5 = FXK == 5;
    constexpr bool PK = FX4;                            // the spans read (and written to the descriptor) as the dwords of the lane's slot block
    const DevFx fx = FX3 ? ps.fx2 : ps.fx;          // (fx2: whichever of the two newer forms the host uploaded)
    // A chunk with fewer rows than the launch has lanes (a 2 MB call: 7 000 rows for 262 144 lanes): the waves that have work are
    // spread over the workgroups -- a wave alone on its CU walks without neighbours at the LDS --, and a workgroup without work (in
    // the fix-up launch: with empty lists) leaves before it stages the tables.
    const bool sparse = !STAGE && a.n < (((uint64_t) gridDim.x * blockDim.x) >> 6) * 64;
    const uint32_t wave_slot = sparse ? wave * gridDim.x + blockIdx.x : (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (a.fix_list != nullptr) {
        bool idle;
        if constexpr (SLOW) {
            // (through a word of the dynamic LDS: a static __shared__ variable would move the tables off LDS address 0)
            LDS_AS uint32_t *flag = (LDS_AS uint32_t *) lds;
            if (threadIdx.x == 0) *flag = 0;
            __syncthreads();
            // (the listed rows are dealt out in batches of 64, batch t to wave t mod waves -- k_fix_prefix, below: a wave has work iff its
            // slot is a batch number)
            // a chunk with fewer rows than the launch has lanes (a 2 MB call): every wave takes what it listed itself, no prefix launch)
            const uint64_t nw_ = ((uint64_t) gridDim.x * blockDim.x) >> 6;
            if (lane == 0 && (sparse ? ((const uint32_t *) a.fix_count)[wave_slot] != 0 : wave_slot < ((const uint32_t *) a.fix_count)[2 * nw_])) *flag = 1;      // (fix_pre[waves]: the batches there are)
            __syncthreads();
            idle = *flag == 0;
            __syncthreads();
        }
        else idle = (uint64_t) (sparse ? blockIdx.x : blockIdx.x * (blockDim.x >> 6)) * 64 >= a.n;       // (its first wave's first row)
        if (idle) {
            if (!SLOW && lane == 0) ((uint32_t *) a.fix_count)[wave_slot] = 0;
            return;
        }
    }
    {
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        const v4u *src = (const v4u *) fx.base;
        LDS_AS v4u *dst = (LDS_AS v4u *) g_lds;
        for (uint32_t i = threadIdx.x; i < fx.bytes / 16; i += blockDim.x) dst[i] = src[i];
        if (a.pg) {
            LDS_AS uint8_t *pg_lds = lds + a.pg_lds_off;
            for (int i = 0; i < a.pg->nrules; i++) {
                if (a.pg->rule_lds_off[i] == 0xFFFFFFFFu) continue;
                const uint8_t *rs = a.pg->rules[i].dfa.cls;
                for (uint32_t k = threadIdx.x; k < a.pg->rule_lds_bytes[i]; k += blockDim.x) pg_lds[a.pg->rule_lds_off[i] + k] = rs[k];
            }
        }
        if (STAGE && a.stage_nbuf && threadIdx.x == 0) *(LDS_AS uint32_t *) (lds + a.stage_lds_off) = (1u << a.stage_nbuf) - 1u;   // every buffer free
        __syncthreads();
    }
    if ((uint32_t) (uintptr_t) lds != 0) __builtin_trap();      // (the walk addresses the tables as LDS addresses: dynamic LDS starts at 0 here)
    // (round 5, measured and not kept: TileCfg's dwords as LANES of two registers, a uniform value = one v_readlane_b32 -- the compiler has
    // no scalar registers left and re-loads the configuration from the kernel arguments inside the phases behind the walk, 41 scalar loads in
    // the field sizes alone.  The stamps showed that phase 10 % shorter, the launch was no shorter: 1.565 against 1.555 ms on one box.)
#define CFG(member) ((uint32_t) a.tc.member)
    // per wave: capture columns [slot][lane] u16, then the lanes' time-text slots.  Lanes l and l + 32 share a dword of a column:
    // an LDS write is served 32 lanes at a time, so the unconditional capture write of a step never meets a bank twice
    LDS_AS uint8_t *wbase = lds + a.tile_lds_off + wave * a.tile_wave_bytes;
    // FX4: a BLOCK of slots per lane instead -- [lane][slot] u16, 68 bytes apart (17 dwords: the 64 lanes' copies of one slot sit in 64
    // different banks) --, so that a slot's address is the block's plus a BYTE of the table cell: one operation per capture write
    constexpr uint32_t CAP_STEP = FX4 ? 2u : FX_CAP_STRIDE;
    LDS_AS uint8_t *capcol = FX4 ? wbase + lane * 68u : wbase + ((lane & 31) << 2) + ((lane >> 5) << 1);
    CapLds capl;
    capl.base = capcol; capl.stride_b = CAP_STEP;
    const uint64_t nwaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    uint16_t *chk = a.chk + ((size_t) wave_slot * a.chk_len) * 64 + lane;
    const uint8_t *data_end = a.data + a.bytes;
    const int ncap = 2 * a.tc.nfields, tc_nfields = a.tc.nfields;
    const bool size_from_columns = !a.cfg.reserve_data && !(a.cfg.preserve_key && !a.cfg.key.is_ra) && a.tc.plain_types;
    const uint32_t klen = (uint32_t) a.cfg.key.key_len;
    const bool fast_layout = !a.cfg.key.is_ra && klen >= 1 && klen <= 15;
    // which of the two plain layouts the burst is aimed at: the one the chunk's first record has (records of the other kind
    // go to the fix-up launch)
    const bool map32 = a.n > 0 && a.row_off[1] - a.row_off[0] > 13 && a.data[a.row_off[0] + 12] == 0xdf;
    const uint32_t vh_at = (map32 ? 23u : 15u) + klen;      // where the value's header sits
    const uint32_t p2_at = fx.off_p2;
    const uint64_t n = a.n;
    uint32_t n_dec = 0, n_gen = 0, n_fin = 0, n_slow = 0, n_loc = 0, pg_out = 0, pg_keep = 0, pg_pending = 0;
    unsigned long long pg_bytes = 0;
    // (the fix-up launch starts at the first flagged row: normally the last two records of the chunk)
    uint32_t trace_it = 0;
    // (bit 31 of trace_iters: the FIX-UP launch is the one that writes its stamps -- FLBGPU_TRACE_FIXUP=1)
    const uint32_t trace_n = a.trace_iters & 0x7FFFFFFFu;
    const bool trace_me = a.trace != nullptr && SLOW == ((a.trace_iters >> 31) != 0);
#define REG_TRACE_(k) if ((k) < 8 && trace_me && trace_it < trace_n) { __builtin_amdgcn_s_waitcnt(0); if (lane == 0) a.trace[((uint64_t) wave_slot * trace_n + trace_it) * 8 + (k)] = __builtin_amdgcn_s_memtime(); }
    // (-DREG_TRACE_FINE, tools/variant.sh: the eight stamps spent behind the walk -- 0 start, 1 walked, 2 result + time text, 3 spans read,
    // 4 fields, 5 rules, 6 time, 7 stores)
#ifdef REG_TRACE_FINE
#define REG_TRACE(k) REG_TRACE_((k) == 0 ? 0 : (k) == 4 ? 1 : (k) >= 5 ? (k) : 8)
#define REG_TRACEF(k) REG_TRACE_(k)
#else
#define REG_TRACE(k) REG_TRACE_(k)
#define REG_TRACEF(k)
#endif
    // the row offsets of an iteration are loaded one iteration ahead (a memory round trip the wave would otherwise sit through
    // at the top of every iteration: 8 k of its 140 k cycles)
    uint64_t po0 = 0, po1 = 0, prow = 0;                                                // (prow: the row those offsets belong to)
    const uint32_t *perm = SLOW ? nullptr : a.perm;
    if constexpr (!SLOW) {
        const uint64_t r0 = (uint64_t) wave_slot * 64 + lane;
        if (r0 < n) { prow = perm ? (uint64_t) perm[r0] : r0; po0 = a.row_off[prow]; po1 = a.row_off[prow + 1]; }
    }
    unsigned long long len_max = 0, len_sum = 0;                                        // (ParserMatchArgs::len_stat)
    const bool len_note = !SLOW && !perm && a.len_stat != nullptr && (wave_slot & 7) == 0;
    // The rows the fast pass leaves to the fix-up launch go onto a LIST, one region per wave (no atomics: a wave numbers its own
    // rows); the fix-up launch has the same shape, and wave w takes the rows wave w listed, 64 per iteration
    const bool listed = a.fix_list != nullptr;
    const uint64_t fix_stride = ((n + nwaves * 64 - 1) / (nwaves * 64)) * 64;           // rows a wave sees at most
    uint32_t *my_fix = listed ? a.fix_list + (uint64_t) wave_slot * fix_stride : nullptr;
    uint32_t *fix_cnt = (uint32_t *) a.fix_count;                                      // [nwaves] rows listed per wave
    uint32_t nfix = 0;                                                                  // fast pass: rows listed so far (uniform)
    // The fix-up launch deals the listed rows out in BATCHES of 64 (round 6): fix_pre[w] = batches of the waves in front of w, batch t is
    // batch t - fix_pre[o] of the wave o that listed it, and wave w of this launch takes the batches w, w + waves, ... -- a wave that
    // listed four batches' worth (rows walked in the order of their lengths put the rows of one layout side by side) no longer holds the
    // launch for four iterations while most waves run two
    const uint32_t *fix_pre = fix_cnt + nwaves;                                         // [nwaves + 1]
    const bool dealt = SLOW && listed && !sparse;
    const uint64_t nloop = (SLOW && listed) ? (dealt ? (uint64_t) fix_pre[nwaves] : (uint64_t) fix_cnt[wave_slot]) : n;
    for (uint64_t base = SLOW ? (listed ? (dealt ? (uint64_t) wave_slot : 0) : (a.fix_first & ~63ull) + (uint64_t) wave_slot * 64) : (uint64_t) wave_slot * 64; base < nloop;
         base += (SLOW && listed) ? (dealt ? nwaves : 64) : nwaves * 64, trace_it++) {
        uint64_t r = base + lane;
        bool act = r < nloop;
        if (SLOW && listed && !dealt) { r = act ? (uint64_t) my_fix[r] : 0; act = act && r < n; }
        if (dealt) {
            uint32_t lo = 0, hi = (uint32_t) nwaves;                                    // fix_pre[lo] <= base < fix_pre[hi]
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (fix_pre[mid] <= (uint32_t) base) lo = mid; else hi = mid; }
            const uint32_t at = ((uint32_t) base - fix_pre[lo]) * 64 + lane;
            act = at < fix_cnt[lo];
            r = act ? (uint64_t) a.fix_list[(uint64_t) lo * fix_stride + at] : 0;
            act = act && r < n;
        }
        REG_TRACE(0)
        if constexpr (SLOW) { act = act && (a.info[r] & RF_NEEDLOC); if (!__ballot(act)) continue; }
        bool to_fix = false;                            // this row goes to the fix-up launch (fast kernel)
        RecInfo ri;
        recinfo_init(ri);
        uint32_t out_len = 0;
        uint64_t o0 = 0, o1 = 0;
        if constexpr (SLOW) { if (act) { o0 = a.row_off[r]; o1 = a.row_off[r + 1]; } }
        else {
            o0 = po0; o1 = po1;
            const uint64_t rn = r + nwaves * 64;                                       // (r: still the lane's PLACE here)
            if (act) r = prow;
            po0 = po1 = 0;
            if (rn < n) { prow = perm ? (uint64_t) perm[rn] : rn; po0 = a.row_off[prow]; po1 = a.row_off[prow + 1]; }
        }
        const uint8_t *recg = a.data + o0;             // (the fast kernel: or its place in the padded copy of the chunk's tail)
        const uint32_t rlen = (uint32_t) (o1 - o0);
        // ---- ONE burst of loads per lane: the first 48 bytes of the record (header, key, value header of the plain layout) and
        // 272 bytes from where the value starts -- all issued before anything is decoded, so that every cache line of the wave's
        // 64 records is requested within one burst (two bursts a few microseconds apart had each line fetched 2.4 times: 72 MB
        // of records are in flight across the chip, the L2 holds 32).  Where the value starts follows from the record's LENGTH
        // for the encoding every producer writes (the smallest str header that holds the length: lib/msgpack-c pack_template.h):
        // a record that spells its value's length another way is decoded like any other layout, by the fix-up launch.
        v4u32 q[18];                                     // bytes 0 .. 271 of the value (q[17]: zero, the walk's read-ahead)
        #pragma unroll
        for (uint32_t k = 0; k < 18; k++) q[k] = (v4u32) (0);
        // (round 5, measured and not kept: q left unset + the loads without the per-lane "inside my record" test -- 72 v_mov and 34 compares
        // less, but the allocator then spills 36 registers instead of 8 and the kernel is 6 % slower)
        // REG_STREAM: only the window being walked and the next one are in registers (q[0..3], pn0..3); the next window's four loads go
        // out when a window's walk starts.  The value's other 192 bytes no longer sit in (spilled) registers.
        v4u32 pn0 = (v4u32) (0), pn1 = (v4u32) (0), pn2 = (v4u32) (0), pn3 = (v4u32) (0);
        constexpr bool STREAMW = REG_STREAM && !SLOW && !STAGE;
        // (the fast kernel reads up to 16 + klen + 288 bytes from the record's start and 96 bytes past a long value's end: the last
        // records of the chunk are read from a zero-padded copy of the chunk's tail instead)
        if constexpr (!SLOW) {
            if (act && recg + rlen + 400 > data_end) recg = (a.tail_buf && o0 >= a.tail_start) ? a.tail_buf + (o0 - a.tail_start) : nullptr;
        }
        const bool try_fast = !SLOW && act && fast_layout && rlen >= vh_at + 2 && rlen < 0x10000u && recg != nullptr;
        // header bytes of the value by its length: fixstr <= 31, str8 <= 255, str16 (rlen < 64 K: no str32 here)
        const uint32_t vspan = rlen - (vh_at + 1);       // header's length bytes + value
        const uint32_t voff_p = vh_at + (vspan <= 31 ? 1u : vspan <= 256 ? 2u : 3u);
        uint32_t hw[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t maxr = wave_umax(try_fast ? rlen : 0);
        if (len_note) { len_max += (unsigned long long) maxr * (unsigned) __builtin_popcountll(__ballot(try_fast)); if (try_fast) len_sum += rlen; }
        REG_TRACE(1)                                    // row offsets arrived
        v4u32 h0 = (v4u32) (0), h1 = (v4u32) (0), h2 = (v4u32) (0);
        bool staged = false;                            // this lane's header and value came through a staging buffer
        if constexpr (STAGE) {
            // ---- staged ingest (FLBGPU_STAGE_NBUF > 0; measured slower than the per-lane burst: with three buffers a CU has 54 KB
            // of the chunk in flight instead of 280 KB, and the memory latency is what bounds the ingest -- kept for the record):
            // the wave's 64 records are ONE contiguous range of the chunk.  Per-lane 16-byte loads at a
            // 277-byte stride ask the L1 for every cache line eight times and, with 280 KB of records in flight per CU, get most
            // of them from the L2 or further again; here the range comes in once, with coalesced 16 B / lane loads, into one of
            // the workgroup's few LDS staging buffers, every lane copies its header and its value into registers (ds_read_b128
            // at its own byte offset), and the buffer goes back to the ring: it is held for one memory round trip, not for the walk.
            const uint32_t cnt = (uint32_t) ((n - base) < 64 ? (n - base) : 64);
            if (a.stage_nbuf && cnt > 0) {
                const uint64_t wend = __shfl(o1, (int) (cnt - 1), 64);
                if (__ballot(try_fast) && wend + 32 <= a.bytes) {
                    LDS_AS uint32_t *smask = (LDS_AS uint32_t *) (lds + a.stage_lds_off);
                    int sbuf = 0;
                    if (lane == 0) {
                        for (;;) {
                            const uint32_t mfree = __hip_atomic_load(smask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (mfree) {
                                const uint32_t bit = mfree & (0u - mfree);
                                if (__hip_atomic_fetch_and(smask, ~bit, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) & bit) { sbuf = __builtin_ctz(bit); break; }
                            }
                            else __builtin_amdgcn_s_sleep(2);
                        }
                    }
                    sbuf = __builtin_amdgcn_readfirstlane(sbuf);
                    LDS_AS uint8_t *sb = lds + a.stage_lds_off + 16 + (uint32_t) sbuf * (a.stage_bytes + STAGE_SLACK);
                    // the records 0 .. m - 1 fit the buffer together (normally all 64; the others take the per-lane loads below)
                    const uint64_t g0 = __shfl(o0, 0, 64);
                    const uint32_t al = (uint32_t) (g0 & 15);                         // (a.data is 16-byte aligned: the host checks)
                    const bool fit = lane < cnt && (o1 - g0) + al <= (uint64_t) a.stage_bytes;
                    const uint64_t fm = __ballot(fit);
                    uint32_t m = (~fm == 0) ? 64 : (uint32_t) __builtin_ctzll(~fm);
                    if (m > cnt) m = cnt;
                    if (m > 0) {
                        const uint32_t total = (uint32_t) (__shfl(o1, (int) (m - 1), 64) - g0) + al;
                        const uint8_t *src = a.data + (g0 - al) + 16 * lane;
                        v4u32 t[STAGE_MAXK];
                        #pragma unroll
                        for (uint32_t k = 0; k < STAGE_MAXK; k++) {
                            t[k] = (v4u32) (0);
                            if (1024 * k + 16 * lane < total) t[k] = *(const v4u32 *) (src + 1024 * k);
                        }
                        #pragma unroll
                        for (uint32_t k = 0; k < STAGE_MAXK; k++) if (1024 * k < total) *(LDS_AS v4u32 *) (sb + 1024 * k + 16 * lane) = t[k];
                        if (lane < m && try_fast) {
                            LDS_AS const uint8_t *rp = sb + al + (uint32_t) (o0 - g0);
                            h0 = lds_ldu128(rp); h1 = lds_ldu128(rp + 16); h2 = lds_ldu128(rp + 32);
                            if (!(a.debug_skip & 2)) {
                                #pragma unroll
                                for (uint32_t k = 0; k < 17; k++) if (vh_at + 1 + 16 * k < maxr && voff_p + 16 * k < rlen) q[k] = lds_ldu128(rp + voff_p + 16 * k);
                            }
                            staged = true;
                        }
                    }
                    if (lane == 0) __hip_atomic_fetch_or(smask, 1u << sbuf, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        if (try_fast) {
            if (!staged) {
                h0 = ldu128(recg); h1 = ldu128(recg + 16); h2 = ldu128(recg + 32);
                if (!(a.debug_skip & 2)) {
                    const uint8_t *sp = recg + voff_p;
                    if constexpr (STREAMW) {
                        #pragma unroll
                        for (uint32_t k = 0; k < 4; k++) if (vh_at + 1 + 16 * k < maxr && voff_p + 16 * k < rlen) q[k] = ldu128(sp + 16 * k);
                        if (vh_at + 1 + 64 < maxr && voff_p + 64 < rlen) pn0 = ldu128(sp + 64);
                        if (vh_at + 1 + 80 < maxr && voff_p + 80 < rlen) pn1 = ldu128(sp + 80);
                        if (vh_at + 1 + 96 < maxr && voff_p + 96 < rlen) pn2 = ldu128(sp + 96);
                        if (vh_at + 1 + 112 < maxr && voff_p + 112 < rlen) pn3 = ldu128(sp + 112);
                    }
                    else {
                    #pragma unroll
                    for (uint32_t k = 0; k < 17; k++) if (vh_at + 1 + 16 * k < maxr && voff_p + 16 * k < rlen) q[k] = ldu128(sp + 16 * k);
                    }
                }
            }
            hw[0] = h0.x; hw[1] = h0.y; hw[2] = h0.z; hw[3] = h0.w; hw[4] = h1.x; hw[5] = h1.y; hw[6] = h1.z; hw[7] = h1.w;
            hw[8] = h2.x; hw[9] = h2.y; hw[10] = h2.z; hw[11] = h2.w;
        }
        REG_TRACE(2)                                    // header + value bytes in registers
        bool qfilled = false;
        if (act) {
            bool fast = false;
            if (try_fast) {
                fast = map32 ? reg_fast_decode<true>(hw, klen, a.cfg.key.key, rlen, a.caps_in_lds, a.chk_len, a.counts, ri, out_len)
                             : reg_fast_decode<false>(hw, klen, a.cfg.key.key, rlen, a.caps_in_lds, a.chk_len, a.counts, ri, out_len);
                // (the burst was aimed at the start the smallest encoding gives: another spelling of the length goes the general way)
                if (fast && ri.val_off != voff_p) { fast = false; recinfo_init(ri); out_len = 0; }
                if (fast) n_dec++;
            }
            if (!fast) {
                if constexpr (SLOW) out_len = a.self ? locate_core_ool(a.self, r, recg, a.data + o1, &n_dec, &ri) : locate_core(a, r, recg, a.data + o1, n_dec, ri);
                else { n_loc++; a.info[r] = RF_NEEDLOC; act = false; to_fix = true; if (!listed) atomicMax(&a.counts[MW_FIX_SPAN], (unsigned long long) (n - r)); }   // the fix-up launch takes the row
            }
            else if ((ri.flags & RF_CAND) && !(a.debug_skip & 2) && !STREAMW) qfilled = true;
        }
        if constexpr (!SLOW) {
            // the flagged rows of this iteration onto the wave's list
            const uint64_t fm = __ballot(to_fix);
            if (fm && listed) {
                if (to_fix) my_fix[nfix + (uint32_t) __builtin_popcountll(fm & ((1ull << lane) - 1ull))] = (uint32_t) r;
                nfix += (uint32_t) __builtin_popcountll(fm);
            }
        }
        const bool cand = act && (ri.flags & RF_CAND);
        const uint32_t vlen = ri.val_len;
        const uint8_t *val = recg + ri.val_off;
        const uint32_t maxlen = wave_umax(cand ? vlen : 0);
        // the first group of four positions that holds some candidate's end of text (here, with every lane of the wave active: the
        // reduction reads lane 63)
        const uint32_t mingrp = wave_umin(cand ? vlen >> 2 : 0xFFFFFFFFu);
        int endb = -1;                                  // >= 0 match end, -1 no match, -2 bytes >= 0x80
        REG_TRACE(3)                                    // decoded, shifted
        if (cand) {
            if constexpr (SLOW) {
                // a record the general walk located: its value with one burst of (guarded) loads of its own
                #pragma unroll
                for (uint32_t k = 0; k < 17; k++) { q[k] = (v4u32) (0); if (16 * k <= maxlen) q[k] = ld16_guard(val + 16 * k, data_end); }
                qfilled = true;
            }
            uint32_t e = fx.start_off, jv = 0;           // jv: the position, kept in a vector register (it is uniform)
            uint32_t ph_ = 0;                            // (FX4: the slot bytes of the step before -- nothing owed yet: slot 0, the dummy)
            typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
            uint32_t p_ = 0xFFFFFFFEu, pp_ = 0;          // (FX5: the positions of the step the pending writes belong to, (j | (j + 1) << 16); see REG_WRITES3)
            const uint32_t gend = vlen >> 2, emask = 0xFFFFFFFFu << (8 * (vlen & 3));   // the group that holds position len, its 0xFF bytes
            // positions 0 .. wend are walked: the end-of-text step included; FX3: one more, for a write carried out of that step
            const uint32_t wend = FX3 ? maxlen + 1 : maxlen;
            const uint32_t nwin = (a.debug_skip & 1) ? 0 : wend / 64 + 1;
            // the four bytes at positions jp .. jp+3: 0xFF from position len on (the end-of-text column)
            // (a scalar test keeps the three vector operations out of the groups in front of the SHORTEST value's end: the walk is bound by
            // the operations a wave issues per step as much as by the read's latency)
#define REG_EOT(wd, jp) if ((uint32_t) ((jp) >> 2) >= mingrp) { asm volatile("" ::: "memory"); /* (a branch, not a select) */ \
                const bool here_ = gend == (uint32_t) ((jp) >> 2); (wd) |= here_ ? emask : 0u; }
            // class * 4 of the four bytes of a dword: ONE operation per byte (shift of a selected byte: SDWA) + the table read
#define REG_B4(dst, wd, SEL) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL : "=v"(dst) : "v"(2u), "v"(wd))
#define REG_LDS32(addr) (*(LDS_AS const uint32_t *) (uintptr_t) (uint32_t) (addr))   /* the tables sit at LDS address 0 (checked at the kernel's start) */
#define REG_CLS(wd, k0, k1, k2, k3) { uint32_t a0_, a1_, a2_, a3_; REG_B4(a0_, wd, "BYTE_0"); REG_B4(a1_, wd, "BYTE_1"); REG_B4(a2_, wd, "BYTE_2"); REG_B4(a3_, wd, "BYTE_3"); \
                k0 = REG_LDS32(a0_); k1 = REG_LDS32(a1_ + (FX4 ? 1024u : 0u)); k2 = REG_LDS32(a2_); k3 = REG_LDS32(a3_ + (FX4 ? 1024u : 0u)); }
            // One step: cell address = (entry's low half) + class * 4 in ONE operation (SDWA add of a selected word) and the table
            // read; a look-ahead cell (or a double write) anywhere in the wave -- about two steps in five -- sends every lane through
            // the cell the next byte selects in the row the entry names (for a plain entry just another cell of a valid row), and only
            // the look-ahead lanes take it.  (Reading that cell in EVERY step instead, to save the test, was measured: 25 % more LDS
            // reads and a 4 % slower kernel.)
#define REG_ROWCELL(dst, ent, col) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(dst) : "v"(ent), "v"(col))
#define REG_STEP(ck, cn)                                                                     \
            {                                                                                \
                uint32_t a_;                                                                 \
                REG_ROWCELL(a_, e, ck);                                                      \
                e = REG_LDS32(a_);                                                           \
                if (__builtin_amdgcn_ballot_w64((int32_t) e < 0)) {                          \
                    REG_ROWCELL(a_, e, cn);                                                  \
                    const uint32_t e2_ = REG_LDS32(a_);                                      \
                    e = (int32_t) e < (int32_t) 0xC0000000u ? e2_ : e;   /* 0x80000000 .. 0xBFFFFFFF: look-ahead */ \
                    if (__builtin_amdgcn_ballot_w64((int32_t) e < 0)) e = fx_pair(e, lds, p2_at, capcol, jv); \
                }                                                                            \
                *(LDS_AS uint16_t *) (capcol + (e >> FX_SLOT_SHIFT)) = (uint16_t) jv;        \
                jv++;                                                                        \
            }
            // FX3 (fx.cpp build_fx3): no special entries.  A cell is 8 bytes -- lo = next row | (slot B * 128) << 16, hi = slot A * 128 --
            // and a step is ONE ds_read_b64 and two unconditional capture writes: slot A takes position j - 1 (the write a look-ahead
            // cell or a double write owed to the byte before), slot B position j.  No test, no branch, no second read on the chain.
#define REG_STEP3(ck)                                                                        \
            {                                                                                \
                uint32_t a_;                                                                 \
                REG_ROWCELL(a_, e, ck);                                                      \
                const uint64_t c8_ = *(LDS_AS const uint64_t *) (uintptr_t) a_;              \
                *(LDS_AS uint16_t *) (capcol + (uint32_t) (c8_ >> 32)) = (uint16_t) (jv - 1u); \
                e = (uint32_t) c8_;                                                          \
                *(LDS_AS uint16_t *) (capcol + (e >> FX_SLOT_SHIFT)) = (uint16_t) jv;        \
                jv++;                                                                        \
            }
            // FX4: two positions per read.  The cell of (row, class of byte j, class of byte j + 1) -- the even byte's table entry is
            // class * ncol * 8, the odd one's class * 8: their sum is the cell's offset in the row -- holds the row behind both (low word)
            // and four slot bytes (high word): positions j - 1, j (step 1), j (step 2's carry), j + 1.
#define REG_STEP4(ce, co)                                                                    \
            {                                                                                \
                const uint32_t a_ = e + (ce) + (co);         /* (v_add3_u32: the cell's low word is the row and nothing else) */ \
                const uint64_t c8_ = *(LDS_AS const uint64_t *) (uintptr_t) a_;              \
                if constexpr (FX5) { REG_WRITES3() pp_ = p_; p_ = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, p_) + (u16x2) (2)); } \
                else { REG_WRITES4() }                                                       \
                e = (uint32_t) c8_; ph_ = (uint32_t) (c8_ >> 32);                            \
                jv += 2;                                                                     \
            }
            // (the address of a slot in ONE operation: the lane's block + a selected byte of the cell -- slot * 2, fx.cpp build_fx3 pairs)
#define REG_SLOT(w, SEL) ({ uint32_t o_; asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL \
                                : "=v"(o_) : "v"((uint32_t) (uintptr_t) capcol), "v"(w)); (LDS_AS uint8_t *) (uintptr_t) o_; })
#define REG_WRITES4()                                                                        \
                *(LDS_AS uint16_t *) REG_SLOT(ph_, "BYTE_0") = (uint16_t) (jv - 3u);          \
                *(LDS_AS uint16_t *) REG_SLOT(ph_, "BYTE_1") = (uint16_t) (jv - 2u);          \
                *(LDS_AS uint16_t *) REG_SLOT(ph_, "BYTE_2") = (uint16_t) (jv - 2u);          \
                *(LDS_AS uint16_t *) REG_SLOT(ph_, "BYTE_3") = (uint16_t) (jv - 1u);
            // FX5 (round 5): three ports -- the step's positions j - 1, j, j + 1 -- and their data in ONE register pair: p_ = (j | (j + 1) << 16)
            // of the step the writes belong to (one v_pk_add_u16 per step), pp_ = the pack of the step before, whose high half IS j - 1.
            // Per 4 bytes: 4 class addresses + 2 cell additions + 6 slot additions + 2 packed additions + 2 shifts (the high halves)
            // = 16 vector operations and 12 LDS operations, against 20 and 14 of the four-port form (whose position constants were six
            // v_mov per 4 bytes).
            // (the compiler spells a store of the high half as a shift and ds_write_b16.  ds_write_b16_d16_hi by inline asm -- one operation
            // less per step -- was measured: 1.84 against 1.67 ms, because the compiler does not count an asm's LDS operation and then waits
            // for the step's OTHER writes to retire before the next cell address may be formed: the chain is that sensitive)
#define REG_W16HI(addr, data) { *(LDS_AS uint16_t *) (addr) = (uint16_t) ((data) >> 16); }
#define REG_WRITES3()                                                                        \
                REG_W16HI(REG_SLOT(ph_, "BYTE_0"), pp_)                                      \
                *(LDS_AS uint16_t *) REG_SLOT(ph_, "BYTE_1") = (uint16_t) p_;                \
                REG_W16HI(REG_SLOT(ph_, "BYTE_2"), p_)
            // (The four writes of a step are issued one step LATE, behind the next step's read -- ph_: the slot bytes of the step before --,
            // so that the chain from read to read is the read and one addition.  With 128 registers this cost 32 more spills and
            // gained nothing (2.02 against 1.96 ms); in the 768-thread build, where nothing is spilled, 1.90 -> 1.85 ms.)
            // one group: the word of the NEXT group comes in (its classes are looked up before this group's steps)
#define REG_GROUP(wnext, jp)                                                                 \
            {                                                                                \
                uint32_t wn_ = (wnext), n0_, n1_, n2_, n3_;                                  \
                REG_EOT(wn_, (jp) + 4)                                                       \
                REG_CLS(wn_, n0_, n1_, n2_, n3_)                                             \
                if constexpr (FX4) { REG_STEP4(c0, c1) REG_STEP4(c2, c3) }                   \
                else if constexpr (FX3) { REG_STEP3(c0) REG_STEP3(c1) REG_STEP3(c2) REG_STEP3(c3) } \
                else { REG_STEP(c0, c1) REG_STEP(c1, c2) REG_STEP(c2, c3) REG_STEP(c3, n0_) } \
                c0 = n0_; c1 = n1_; c2 = n2_; c3 = n3_;                                      \
            }
            // The tail of the pattern (dev.hpp DevFx::tail_min): every 16 positions the wave looks whether all its lanes stand in the
            // tail's rows or in an absorbing row; then nothing is left to walk -- a lane with a kill byte in what was skipped goes the
            // way of the poisoned records.  Values that continue in memory windows (>= 272 bytes) are walked in full: the scan for
            // kill bytes reads the registers.
            // REG_TAIL_EXIT: true when the wave may stop here
            const uint32_t tail_min = fx.tail_min;
            const bool tail_allow = !SLOW && !FX3 && !STREAMW && maxlen < 272 && !(a.debug_skip & 128);
#define REG_TAIL_EXIT() (tail_allow && !__builtin_amdgcn_ballot_w64((e & FX_ROW_MASK) < tail_min))
            for (uint32_t c = 0; c < fx.nslots; c++) *(LDS_AS uint16_t *) (capcol + c * CAP_STEP) = 0xFFFF;
            #pragma unroll 1
            for (uint32_t w = 0; w < nwin; w++) {
                v4u32 w0, w1, w2, w3;
                uint32_t nx;                               // first dword of the next window
                if constexpr (STREAMW) {
                    // this window (q[0..3]) while the window behind the next one is requested: its first dword closes this window's last group
                    w0 = q[0]; w1 = q[1]; w2 = q[2]; w3 = q[3]; nx = pn0.x;
                    q[0] = pn0; q[1] = pn1; q[2] = pn2; q[3] = pn3;
                    const uint32_t nb = 64 * (w + 2);
                    const uint8_t *p = val + nb;
                    pn0 = pn1 = pn2 = pn3 = (v4u32) (0);
                    if (w + 2 < nwin && nb <= vlen + 16) { pn0 = ldu128(p); pn1 = ldu128(p + 16); pn2 = ldu128(p + 32); pn3 = ldu128(p + 48); }
                }
                else if (w == 0) { w0 = q[0]; w1 = q[1]; w2 = q[2]; w3 = q[3]; nx = q[4].x; }
                else if (w == 1) { w0 = q[4]; w1 = q[5]; w2 = q[6]; w3 = q[7]; nx = q[8].x; }
                else if (w == 2) { w0 = q[8]; w1 = q[9]; w2 = q[10]; w3 = q[11]; nx = q[12].x; }
                else if (w == 3) { w0 = q[12]; w1 = q[13]; w2 = q[14]; w3 = q[15]; nx = q[16].x; }
                else if (w == 4 && maxlen < 272) { w0 = q[16]; w1 = w2 = w3 = (v4u32) (0); nx = 0; }
                else {
                    // a long value: this window from memory (the loads of a wave go out together; no read-ahead)
                    const uint8_t *p = val + 64 * w;
                    if constexpr (SLOW) {
                        w0 = ld16_guard(p, data_end); w1 = ld16_guard(p + 16, data_end); w2 = ld16_guard(p + 32, data_end); w3 = ld16_guard(p + 48, data_end);
                        nx = ld16_guard(p + 64, data_end).x;
                    }
                    else if (64 * w <= vlen + 16) { w0 = ldu128(p); w1 = ldu128(p + 16); w2 = ldu128(p + 32); w3 = ldu128(p + 48); nx = ldu32(p + 64); }
                    else { w0 = w1 = w2 = w3 = (v4u32) (0); nx = 0; }
                }
                const uint32_t jb = 64 * w;
                uint32_t c0, c1, c2, c3;
                { uint32_t wd = w0.x; REG_EOT(wd, jb) REG_CLS(wd, c0, c1, c2, c3) }
                // (positions 0 .. maxlen are walked: a quarter of a window behind the longest value's end-of-text step nothing is left to
                // do -- a scalar test; without it a 256-byte line pays a fifth window of 64 steps for its one end-of-text step)
                REG_GROUP(w0.y, jb) REG_GROUP(w0.z, jb + 4) REG_GROUP(w0.w, jb + 8) REG_GROUP(w1.x, jb + 12)
                if (jb + 16 > wend || REG_TAIL_EXIT()) break;
                REG_GROUP(w1.y, jb + 16) REG_GROUP(w1.z, jb + 20) REG_GROUP(w1.w, jb + 24) REG_GROUP(w2.x, jb + 28)
                if (jb + 32 > wend || REG_TAIL_EXIT()) break;
                REG_GROUP(w2.y, jb + 32) REG_GROUP(w2.z, jb + 36) REG_GROUP(w2.w, jb + 40) REG_GROUP(w3.x, jb + 44)
                if (jb + 48 > wend || REG_TAIL_EXIT()) break;
                REG_GROUP(w3.y, jb + 48) REG_GROUP(w3.z, jb + 52) REG_GROUP(w3.w, jb + 56) REG_GROUP(nx, jb + 60)
                if (REG_TAIL_EXIT()) break;
            }
            if constexpr (FX5) { REG_WRITES3() }
            else if constexpr (FX4) { REG_WRITES4() }
            // ---- lanes that stand in the tail with text left: positions jv .. vlen - 1 were not walked
            bool tail_kill = false;
            {
                const uint32_t T = (uint32_t) __builtin_amdgcn_readfirstlane((int) jv);
                const bool in_tail = (e & FX_ROW_MASK) >= tail_min && (e & FX_ROW_MASK) < fx.absorb_off && T <= vlen;
                if (tail_allow && __builtin_amdgcn_ballot_w64(in_tail)) {
                    uint32_t bad = 0;
                    if (T < maxlen) {
                        const uint32_t kx0 = fx.kill[0] * 0x01010101u, kx1 = fx.kill[1] * 0x01010101u, kx2 = fx.kill[2] * 0x01010101u;
                        reg_kill_scan<0>(q, T >> 2, (maxlen - 1) >> 2, vlen, fx.nkill, kx0, kx1, kx2, bad);
                    }
                    // a kill byte in what was skipped (a byte >= 0x80 would have met the poison row; a line feed is the other one in
                    // practice): the record takes the way of the poisoned ones -- the generic kernel runs the complete algorithm
                    tail_kill = in_tail && bad != 0;
                    if (in_tail && !tail_kill) {
                        // the row a lane stands in is as good as the one it would have reached: the last byte decides (its entry, with the
                        // end of the text behind it for a look-ahead cell), then the end-of-text step
                        const uint32_t eotc = fx.ncls1 * 4u - 4u;                       // the end-of-text column (ncls * 4)
                        if (vlen > T) {
                            const uint32_t lb = ld8(val + vlen - 1);
                            e = REG_LDS32((e & FX_ROW_MASK) + REG_LDS32(lb * 4u));
                            if ((int32_t) e < 0) {
                                if ((int32_t) e < (int32_t) 0xC0000000u) e = REG_LDS32((e & FX_ROW_MASK) + eotc);
                                e = fx_pair(e, lds, p2_at, capcol, vlen - 1);
                            }
                            *(LDS_AS uint16_t *) (capcol + (e >> FX_SLOT_SHIFT)) = (uint16_t) (vlen - 1);
                        }
                        e = REG_LDS32((e & FX_ROW_MASK) + eotc);
                        e = fx_pair(e, lds, p2_at, capcol, vlen);
                        *(LDS_AS uint16_t *) (capcol + (e >> FX_SLOT_SHIFT)) = (uint16_t) vlen;
                    }
                }
            }
#undef REG_TAIL_EXIT
#undef REG_GROUP
#undef REG_STEP3
#undef REG_STEP4
#undef REG_WRITES4
#undef REG_WRITES3
#undef REG_W16HI
#undef REG_SLOT
#undef REG_STEP
#undef REG_ROWCELL
#undef REG_CLS
#undef REG_LDS32
#undef REG_B4
#undef REG_EOT
            const uint32_t S = e & FX_ROW_MASK;
            const uint32_t e_eot = capl.get((uint32_t) ncap + FXS_END_EOT - 1), e_mid = capl.get((uint32_t) ncap + FXS_END_MID - 1),
                           d_eot = capl.get((uint32_t) ncap + FXS_DEAD_EOT - 1), failed = capl.get((uint32_t) ncap + FXS_FAIL - 1);
            int res;                                    // 1 match, 0 no match at boundary 0 / undecided, -2 poison
            if (S == fx.poison_off || tail_kill) res = -2;
            else if (failed != CAP_UNSET) res = 0;
            else if (e_mid != CAP_UNSET) { res = 1; endb = (int) e_mid; }
            else if (e_eot != CAP_UNSET) { if (e_eot == vlen) { res = 1; endb = (int) vlen; } else res = -2; }
            else if (d_eot != CAP_UNSET) res = d_eot == vlen ? 0 : -2;
            else res = 0;
            if (res == -2) endb = -2;
            else if (res == 0 && !(a.debug_skip & 1)) {
                // a later start (line anchors), cells that need the reverse pass' viable sets, or no match at all
                n_slow++;
                if constexpr (SLOW) endb = tile_capture_slow(&ps, val, vlen, chk, capcol, CAP_STEP);
                else endb = -2;                                                  // the generic kernel runs the complete algorithm
            }
            if (a.debug_skip & 4) endb = -1;
        }
        REG_TRACE(4)                                    // walked
        // the time field's text out of the value's registers, first thing behind the walk: while nothing else is live the barrel
        // shifter (40 + 24 + 16 + 12 + 10 + 9 selects) fits beside the value's 68 registers
        RegTimeText tt;
        #pragma unroll
        for (int k = 0; k < 8; k++) tt.w[k] = 0;
        bool tt_ok = false;
        const int c_tf = (int) CFG(time_field);
        if (cand && endb >= 0 && qfilled && c_tf >= 0 && CFG(plan.ok) && !CFG(defer_time) && !(a.debug_skip & 64)) {
            const uint32_t tb0 = capl.get((uint32_t) (2 * c_tf)), te0 = capl.get((uint32_t) (2 * c_tf + 1));
            if (tb0 != CAP_UNSET && te0 != CAP_UNSET && te0 - tb0 == CFG(plan.len) && te0 - tb0 <= 4 * TBUF_WORDS && tb0 + 32 <= 272) {
                reg_text<8>(q, tb0, tt.w);
                tt_ok = true;
            }
        }
        // the first rule's field out of the value's registers, right behind the walk like the time text (nothing else is live yet): the
        // line a load would ask for here has left the L2 as often as not -- the kernel is 40 k cycles and 7.5 MB per XCD further
        RuleText rt{-1, 0, (v4u32) (0)};
        uint32_t ytext_q = 0, ytb = 0xFFFFFFFFu;        // the year's four digits (time lookup left to k_pg_emit) and the span begin they were taken at
        if constexpr (!SLOW && PK) {
            if (cand && endb >= 0 && qfilled && c_tf >= 0 && CFG(defer_time)) {
                const uint32_t tb0 = capl.get((uint32_t) (2 * c_tf));
                if (tb0 != CAP_UNSET && tb0 + CFG(year_off) <= 59) { ytb = tb0; ytext_q = reg_dword_head(q, tb0 + CFG(year_off)); }
            }
            const int rf = (a.pg_keep_len && CFG(pg_on) && a.tc.pg_fast && a.tc.pg_nrules > 0 && a.tc.rule[0].fmask) ? 31 - (int) __builtin_clz(a.tc.rule[0].fmask) : -1;
            if (cand && endb >= 0 && qfilled && rf >= 0) {
                const uint32_t rb = capl.get((uint32_t) (2 * rf));
                if (rb <= 272u - 32u) {
                    uint32_t w4[4];
                    reg_text<4>(q, rb, w4);
                    rt.f = rf; rt.b = rb; rt.w.x = w4[0]; rt.w.y = w4[1]; rt.w.z = w4[2]; rt.w.w = w4[3];
                }
            }
        }
        REG_TRACEF(2)
        if (act) {
            uint32_t flags = ri.flags;
            bool done = false;                           // the row is complete: parsed, sized, (pair mode) decided
            bool caps_valid = false, will_finish = false;
            uint32_t keep_len = PG_UNDECIDED;
            uint64_t null_mask = 0;
            uint32_t cdw[17];                            // FX4: the lane's slot block as dwords (read once for the fields, again in the descriptor)
            #pragma unroll
            for (int k = 0; k < 17; k++) cdw[k] = 0xFFFFFFFFu;
            if (cand && endb >= 0) {
                flags |= RF_RXOK;
                caps_valid = true;
                // ---- named fields, time, size (k_parser_finish's fast path); pair mode: the rules (k_parser_rx's block).
                // Everything about the parser and the rules comes from the kernel arguments (TileCfg: scalar loads).
                const TileCfg &tc = a.tc;
                bool any = false, slow = !size_from_columns, time_here = false;
                uint32_t kept = 0, drop = 0, body_bytes = 0, pgdrop = CFG(pg_static_drop), tb = 0, tfl = 0;
                int64_t sec = 0;
                // (the per-lane slot block, FX4: a span comes out of the block's dwords as it is stored -- u16, 0xFFFF = unset)
                constexpr uint32_t UNSET = PK ? 0xFFFFu : CAP_UNSET;
                // (straight-line for the fields that are not time keys: the lambda's early returns had compiled into a tree of
                // exec-mask branches per field, round 5)
                const uint32_t c_skip = CFG(skip_empty), c_tmask = CFG(is_time_mask);
                auto field = [&](int f, uint32_t b, uint32_t e) {
                    const bool set = b != UNSET && e != UNSET;
                    any |= set;
                    const uint32_t fl = set ? e - b : 0;
                    const bool emp = fl == 0 && c_skip != 0;
                    const uint32_t bit = emp ? 1u << f : 0u;
                    drop |= bit; pgdrop |= bit;
                    const uint32_t nc = (uint32_t) tc.name_cost[f];
                    // (fl < 65536: a candidate's value is shorter than 0xFFFF bytes, reg_fast_decode / locate_core)
                    const uint32_t cost = nc + 1u + fl + (fl >= 32 ? 1u : 0u) + (fl >= 256 ? 1u : 0u);
                    if ((c_tmask >> f) & 1) {                             // (uniform)
                        if (!emp) {
                            // the fixed-layout plan or k_parser_finish's interpreter (a text of another length, several time fields, ...)
                            if (f == c_tf && CFG(plan.ok) && fl == CFG(plan.len) && fl <= 4 * TBUF_WORDS) {
                                time_here = true; tb = b; tfl = fl;
                                if (!CFG(time_keep)) drop |= 1u << f;
                                else { kept++; body_bytes += cost; }
                            }
                            else slow = true;
                        }
                        return;
                    }
                    body_bytes += emp ? 0u : cost;
                    kept += emp ? 0u : 1u;
                };
                {
                    // the spans of the first 16 fields in ONE batch of LDS reads (each read waits behind the other waves' walks:
                    // 18 of them one after the other were a fifth of the time behind the walk)
                    uint32_t cb[16], ce[16];
                    if constexpr (PK) {
                        // the lane's block [slot] u16 (slot 0 the dummy, span c in slot c + 1): dword k = slots 2 k, 2 k + 1 = (end of
                        // field k - 1, begin of field k) -- up to five reads instead of two per field
                        const uint32_t nd = (uint32_t) tc_nfields + 1;           // dwords that hold the named fields' spans (uniform)
                        const v4u32 s0 = lds_ldu128(capcol);
                        v4u32 s1 = (v4u32) (0xFFFFFFFFu), s2 = (v4u32) (0xFFFFFFFFu), s3 = (v4u32) (0xFFFFFFFFu);
                        if (nd > 4) s1 = lds_ldu128(capcol + 16);
                        if (nd > 8) s2 = lds_ldu128(capcol + 32);
                        if (nd > 12) s3 = lds_ldu128(capcol + 48);
                        if (nd > 16) cdw[16] = *(LDS_AS const uint32_t *) (capcol + 64);
                        cdw[0] = s0.x; cdw[1] = s0.y; cdw[2] = s0.z; cdw[3] = s0.w; cdw[4] = s1.x; cdw[5] = s1.y; cdw[6] = s1.z; cdw[7] = s1.w;
                        cdw[8] = s2.x; cdw[9] = s2.y; cdw[10] = s2.z; cdw[11] = s2.w; cdw[12] = s3.x; cdw[13] = s3.y; cdw[14] = s3.z; cdw[15] = s3.w;
                        #pragma unroll
                        for (int f = 0; f < 16; f++) { cb[f] = cdw[f] >> 16; ce[f] = cdw[f + 1] & 0xFFFFu; }
                    }
                    else {
                    #pragma unroll
                    for (int f = 0; f < 16; f++) {
                        cb[f] = CAP_UNSET; ce[f] = CAP_UNSET;
                        if (f < tc_nfields) { cb[f] = capl.get((uint32_t) (2 * f)); ce[f] = capl.get((uint32_t) (2 * f + 1)); }
                    }
                    }
                    REG_TRACEF(3)
                    #pragma unroll
                    for (int f = 0; f < 16; f++) if (f < tc_nfields) field(f, cb[f], ce[f]);
                    for (int f = 16; f < tc_nfields; f++) field(f, capl.get((uint32_t) (2 * f)) & UNSET, capl.get((uint32_t) (2 * f + 1)) & UNSET);
                }
                REG_TRACEF(4)
                // pair mode with the time lookup left to k_pg_emit (TileCfg::defer_time): the year's four digits, requested here and
                // looked at behind the rules
                // (the fix-up launch keeps the lookup: its rows are few, and its register budget is spent)
                uint32_t ytext = 0;
                const bool ycheck = !SLOW && CFG(defer_time) && time_here && !(flags & RF_BADTS);
                if (ycheck) {
                    // (from the value's registers when the digits sit in its first 64 bytes -- a load here fetched the line again, from HBM
                    // as often as not: + 0.8 GB of FETCH per 10 M records, round 5)
                    if (ytb == tb) ytext = ytext_q;                      // (taken right behind the walk, with the rule's field)
                    else ytext = ldu32(val + tb + CFG(year_off));
                }
                auto text_from_memory = [&]() {
                    const v4u32 t0 = load16(val + tb, 0, tfl), t1 = load16(val + tb + 16, 0, tfl > 16 ? tfl - 16 : 0);
                    tt.w[0] = t0.x; tt.w[1] = t0.y; tt.w[2] = t0.z; tt.w[3] = t0.w; tt.w[4] = t1.x; tt.w[5] = t1.y; tt.w[6] = t1.z; tt.w[7] = t1.w;
                };
                if constexpr (SLOW) { if (time_here && !tt_ok && !(a.debug_skip & 64)) text_from_memory(); }
                uint32_t pgbits = 0;
                if (CFG(pg_on) && any && !(CFG(pg_named) & CFG(pg_time_fields) & ~pgdrop) && !(a.debug_skip & 16)) {
                    TileCaps cv{capl};
                    LDS_AS const uint8_t *pg_lds = (LDS_AS const uint8_t *) (lds + a.pg_lds_off);
                    const bool keep = tc.pg_fast ? tc_grep_parsed<!SLOW>(tc, a.pg->rules, pgdrop, val, cv, pg_lds, rt)
                                                 : pg_grep_parsed<true>(a.pg->rules, a.pg->nrules, a.pg->logical_op, a.pg->rule_fmask, a.pg->rule_lds_off, pgdrop, val, cv, pg_lds);
                    pgbits = RF_PGDONE | (keep ? RF_PGKEEP : 0u);
                }
                bool defer = false;
                if (ycheck && (pgbits & RF_PGDONE) && !slow) {
                    const uint32_t t7 = ytext & 0x7F7F7F7Fu, isd = (t7 + 0x50505050u) & ~(t7 + 0x46464646u) & ~ytext & 0x80808080u;
                    const uint32_t year = (ytext & 15u) * 1000u + ((ytext >> 8) & 15u) * 100u + ((ytext >> 16) & 15u) * 10u + ((ytext >> 24) & 15u);
                    defer = isd == 0x80808080u && year >= 1971u && year <= 2105u;
                }
                // the time text: taken out of the value's registers right behind the walk (tt_ok); a text that reaches behind byte 272
                // of a long value: two loads
                if constexpr (!SLOW) { if (time_here && !defer && !tt_ok && !(a.debug_skip & 64)) text_from_memory(); }
                REG_TRACE(5)                            // fields, rules
                if (defer) pgbits |= RF_TIMEPEND;
                if (time_here && !defer && !(a.debug_skip & 32)) {
                    int64_t s2 = 0;
                    bool tok;
                    if constexpr (FX3) {
                        LDS_AS const uint32_t *ctp = (LDS_AS const uint32_t *) (lds + (fx.bytes - 128u));
                        tok = ctp[31] ? time_fast_compiled(ctp, (int) CFG(time_with_tz), (int) CFG(time_offset), tt.w, &s2) : time_fast_plan(tc.plan, tc.time_with_tz, tc.time_offset, tt, &s2);
                    }
                    else tok = time_fast_plan(tc.plan, tc.time_with_tz, tc.time_offset, tt, &s2);
                    if (tok) sec = s2;
                    else slow = true;
                }
                REG_TRACE(6)                            // time
                flags |= pgbits;
                if (!any) {
                    // flb_regex_parse found no participating named group: the parser fails (k_parser_finish)
                    if (a.cfg.nparsers > 1) { flags |= RF_GENERIC; n_gen++; }
                }
                else if (slow) {
                    // k_parser_finish takes over: it reads the spans and the time text from the columns
                    n_fin++;
                    will_finish = true;
                    if (tc.time_field >= 0) {
                        const uint32_t tb2 = capl.get((uint32_t) (2 * tc.time_field)), te = capl.get((uint32_t) (2 * tc.time_field + 1));
                        if (tb2 != CAP_UNSET && te != CAP_UNSET && te - tb2 <= 4 * TBUF_WORDS) {
                            const uint32_t tl = te - tb2;
                            v4u32 w0 = load16(val + tb2, 0, tl), w1 = load16(val + tb2 + 16, 0, tl > 16 ? tl - 16 : 0);
                            a.tbuf[0 * n + r] = w0.x; a.tbuf[1 * n + r] = w0.y; a.tbuf[2 * n + r] = w0.z; a.tbuf[3 * n + r] = w0.w;
                            a.tbuf[4 * n + r] = w1.x; a.tbuf[5 * n + r] = w1.y; a.tbuf[6 * n + r] = w1.z; a.tbuf[7 * n + r] = w1.w;
                        }
                    }
                }
                else {
                    done = true;
                    if (!a.cfg.key.is_ra) null_note(a.cfg, r, ri.key_index, null_mask);
                    int64_t tsec = ri.ts_sec, tnsec = ri.ts_nsec;
                    if (flags & RF_BADTS) { tsec = -3; tnsec = 0; }                     // the event time was out of range
                    if (sec != 0) { tsec = sec; tnsec = 0; }                            // (the fixed-layout formats carry no fraction)
                    flags = (flags | RF_PARSED) & ~(uint32_t) RF_BADTS;
                    ri.parser_idx = 0; ri.nkept = kept; ri.drop_mask = drop;
                    // encoder timestamp check (src/flb_log_event_encoder.c:345-363)
                    if (encoder_refuses_time(tsec, tnsec)) {
                        flags |= RF_BADTS;
                        out_len = 0;
                        keep_len = 0;
                    }
                    else {
                        ri.ts_sec = (uint32_t) tsec; ri.ts_nsec = (uint32_t) tnsec;
                        // a parsed time of -1 s / -2 s (or 2106-02-07 06:28:14 / :15 UTC): filter_parser writes ff ff ff ff / fe .. as the
                        // timestamp, which the NEXT filter's decoder reads as a group marker -- hidden, or with nanoseconds a decoder error
                        // (src/flb_log_event_decoder.c: kdev.inc decode_event).  Counted (counts[MW_TIME_MARKER]): flb_filter_do's re-count of the filter's
                        // output does not see such a record (src/flb_filter.c:272, src/flb_mp.c:49-71), and the pair, which does not restate
                        // the next decoder's view, hands the chunk to the unfused kernels (flbgpu.cpp run_pair_fused).
                        if ((uint32_t) tsec >= 0xfffffffeu) atomicAdd(&a.counts[MW_TIME_MARKER], 1ull);
                        const uint32_t n0 = CFG(nregs_minus1);
                        out_len = 12 + ri.meta_canon + (n0 < 16 ? 1 : n0 < 65536 ? 3 : 5) + body_bytes;
                        if (a.pg_keep_len) {
                            if (pgbits & RF_PGDONE) {
                                const bool keep = (pgbits & RF_PGKEEP) != 0;
                                keep_len = keep ? out_len : 0;
                                pg_out++; pg_bytes += out_len; pg_keep += keep ? 1u : 0u;
                            }
                            else pg_pending++;
                        }
                    }
                }
            }
            else if (cand && (endb == -2 || a.cfg.nparsers > 1)) {
                // a byte >= 0x80 (UTF-8 tables) or more parsers to try: the generic kernel takes over
                flags |= RF_GENERIC;
                n_gen++;
            }
            ri.flags = flags;
            // ---- columns: what a later kernel reads of this row
            if (!done) {
                // k_parser_finish's treatment of a row it does not parse; a row it will finish itself (will_finish) is left alone
                if (!will_finish) {
                    if (!(flags & RF_GENERIC)) a.null_mask[r] = 0;
                    if (a.pg_keep_len) { a.pg_keep_len[r] = PG_UNDECIDED; pg_pending++; }
                }
                rec_store(a.info, n, r, ri);
                a.out_len[r] = out_len;
                if (caps_valid) for (int c = 0; c < ncap; c++) a.caps[(uint64_t) c * n + r] = capl.get((uint32_t) c);
            }
            else {
                const bool dropped = a.pg_keep_len && keep_len == 0 && !(a.debug_skip & 8);      // pair mode, settled, not kept: nothing reads the rest
                if (a.pg_keep_len) a.pg_keep_len[r] = keep_len;
                if (dropped) a.info[r] = flags;
                else if (a.desc && a.pg_keep_len && keep_len != PG_UNDECIDED) {
                    // kept by the pair: the record's fields as one descriptor (whole sectors, 16 bytes per store)
                    a.info[r] = flags | RF_DESC;
                    v4u32 *dp = (v4u32 *) (a.desc + (uint64_t) r * a.dstride);
                    v4u32 d0; d0.x = ri.ts_sec; d0.y = ri.ts_nsec; d0.z = ri.val_off; d0.w = ri.drop_mask;
                    dp[0] = d0;
                    if constexpr (PK) {
                        // the spans from the block's dwords read for the fields: spans (2 f, 2 f + 1) = the high half of dword f and the low
                        // half of dword f + 1 -- one v_alignbit per descriptor dword, no LDS read
                        #pragma unroll
                        for (uint32_t k = 1; k < 8; k++) {
                            if (4 * k >= a.dstride) break;                 // (uniform)
                            uint32_t wv[4];
                            #pragma unroll
                            for (uint32_t j = 0; j < 4; j++) {
                                const uint32_t di = 4 * k + j;             // dword of the descriptor
                                if (di == 4) wv[j] = ri.meta_off;
                                else if (di == 5) wv[j] = ri.meta_len;
                                else if (di == 6) wv[j] = ri.nkept;
                                else {
                                    const uint32_t f = di - 7;
                                    wv[j] = (f < 16 && (int) f < tc_nfields) ? __builtin_amdgcn_alignbit(cdw[f + 1 <= 16 ? f + 1 : 16], cdw[f <= 16 ? f : 16], 16) : 0xFFFFFFFFu;
                                }
                            }
                            v4u32 dv; dv.x = wv[0]; dv.y = wv[1]; dv.z = wv[2]; dv.w = wv[3];
                            dp[k] = dv;
                        }
                    }
                    else
                    for (uint32_t k = 1; 4 * k < a.dstride; k++) {
                        uint32_t wv[4];
                        #pragma unroll
                        for (uint32_t j = 0; j < 4; j++) {
                            const uint32_t di = 4 * k + j;                 // dword of the descriptor
                            if (di == 4) wv[j] = ri.meta_off;
                            else if (di == 5) wv[j] = ri.meta_len;
                            else if (di == 6) wv[j] = ri.nkept;
                            else {
                                const uint32_t c = 2 * (di - 7);           // spans c, c + 1 as u16
                                const uint32_t lo16 = (int) c < ncap ? capl.get(c) & 0xFFFFu : 0xFFFFu, hi16 = (int) (c + 1) < ncap ? capl.get(c + 1) & 0xFFFFu : 0xFFFFu;
                                wv[j] = lo16 | (hi16 << 16);
                            }
                        }
                        v4u32 dv; dv.x = wv[0]; dv.y = wv[1]; dv.z = wv[2]; dv.w = wv[3];
                        dp[k] = dv;
                    }
                }
                else {
                    rec_store(a.info, n, r, ri);
                    a.null_mask[r] = null_mask;
                    a.out_len[r] = out_len;
                    for (int c = 0; c < ncap; c++) a.caps[(uint64_t) c * n + r] = capl.get((uint32_t) c);
                }
            }
        }
        REG_TRACE(7)                                    // columns stored
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_dec += __shfl_down(n_dec, o, 64); n_gen += __shfl_down(n_gen, o, 64); n_fin += __shfl_down(n_fin, o, 64); n_slow += __shfl_down(n_slow, o, 64);
        n_loc += __shfl_down(n_loc, o, 64);
        pg_out += __shfl_down(pg_out, o, 64); pg_keep += __shfl_down(pg_keep, o, 64); pg_pending += __shfl_down(pg_pending, o, 64);
        pg_bytes += __shfl_down(pg_bytes, o, 64);
    }
    if (!SLOW && listed && lane == 0) fix_cnt[wave_slot] = nfix;
    if (len_note) {
        for (int o = 32; o > 0; o >>= 1) len_sum += __shfl_down(len_sum, o, 64);
        // (a.len_stat = &counts[MW_LEN_STEPS]: len_stat[0] is that slot, len_stat[1] the one behind it, MW_LEN_BYTES)
        if (lane == 0 && len_sum) { atomicAdd(&a.len_stat[0], len_max); atomicAdd(&a.len_stat[1], len_sum); }
    }
    if (lane == 0) {
        if (n_dec) atomicAdd(&a.counts[MW_DECODED], (unsigned long long) n_dec);
        if (n_gen) atomicAdd(&a.counts[MW_GENERIC], (unsigned long long) n_gen);
        if (n_fin) atomicAdd(&a.counts[MW_FINISH], (unsigned long long) n_fin);
        if (n_slow) atomicAdd(&a.counts[MW_SLOW], (unsigned long long) n_slow);
        if (n_loc) atomicAdd(&a.counts[MW_NEEDLOC], (unsigned long long) n_loc);
        if (pg_bytes) atomicAdd(&a.counts[MW_PG_BYTES], pg_bytes);
        if (pg_keep) atomicAdd(&a.counts[MW_PG_KEEP], (unsigned long long) pg_keep);
        if (pg_out) atomicAdd(&a.counts[MW_PG_OUT], (unsigned long long) pg_out);
        if (pg_pending) atomicAdd(&a.counts[MW_PG_PENDING], (unsigned long long) pg_pending);
    }
}
#undef CFG
#undef REG_TRACE
#undef REG_TRACEF
#undef REG_TRACE_
#undef REG_HB

// fix_cnt[nw] rows listed per wave of the fast pass -> fix_pre[nw + 1] (behind them): batches of 64 in front of every wave, the total last
__global__ void __launch_bounds__(1024) k_fix_prefix(uint32_t *fix_cnt, uint32_t nw) {
    __shared__ uint32_t wsum[16];
    uint32_t *pre = fix_cnt + nw;
    const uint32_t per = (nw + 1023) / 1024, i0 = threadIdx.x * per;
    uint32_t mine = 0;
    for (uint32_t i = i0; i < i0 + per && i < nw; i++) mine += (fix_cnt[i] + 63) / 64;
    uint32_t incl = mine;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= (uint32_t) o) incl += t; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (uint32_t w = 0; w < wave; w++) before += wsum[w];
    for (uint32_t i = i0; i < i0 + per && i < nw; i++) { pre[i] = before; before += (fix_cnt[i] + 63) / 64; }
    if (threadIdx.x == 1023) pre[nw] = before;
}

void launch_parser_reg(const ParserMatchArgs &a, int grid, int threads, bool fixup, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, false, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<true, false, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<true, false, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, false, 3, 768>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, false, 4, 768>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, false, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<true, false, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<false, false, 5, 768>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<true, false, 4, 768>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_parser_reg<true, false, 5, 768>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    // (the fix-up pass of a launch of up to 768 threads: its own 768-thread build, 168 registers -- the 1024-thread one keeps 128 and spills
    // 225 of what its general locate wants, round 6; the other table forms keep the 1024-thread build.  Measured and not kept: the same
    // waves as workgroups of 512 threads, 256 registers, nothing spilled -- a CU then holds one such workgroup, the launch needs two rounds)
    if (getenv("FLBGPU_DEBUG_LDS")) fprintf(stderr, "k_parser_reg%s: grid %d x %d threads, lds_total %u, tables up to %u, %u a wave, fx2 %u\n", fixup ? " (fix-up)" : "", grid, threads, a.lds_total, a.tile_lds_off, a.tile_wave_bytes, a.use_fx2);
    if (fixup && a.fix_list && a.n >= (uint64_t) grid * (uint64_t) threads) hipLaunchKernelGGL(k_fix_prefix, dim3(1), dim3(1024), 0, st, (uint32_t *) a.fix_count, (uint32_t) (((uint64_t) grid * (uint64_t) threads) >> 6));
    static const bool fix768 = !(getenv("FLBGPU_FIXUP_1024") && atoi(getenv("FLBGPU_FIXUP_1024")) != 0);
    if (a.use_fx2 == 5) {
        if (fixup && threads <= 768 && fix768) hipLaunchKernelGGL((k_parser_reg<true, false, 5, 768>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else if (fixup) hipLaunchKernelGGL((k_parser_reg<true, false, 5>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else if (threads <= 768) hipLaunchKernelGGL((k_parser_reg<false, false, 5, 768>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else hipLaunchKernelGGL((k_parser_reg<false, false, 5>), dim3(grid), dim3(threads), a.lds_total, st, a);
        return;
    }
    if (a.use_fx2 == 4) {
        if (fixup && threads <= 768 && fix768) hipLaunchKernelGGL((k_parser_reg<true, false, 4, 768>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else if (fixup) hipLaunchKernelGGL((k_parser_reg<true, false, 4>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else if (threads <= 768) hipLaunchKernelGGL((k_parser_reg<false, false, 4, 768>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else hipLaunchKernelGGL((k_parser_reg<false, false, 4>), dim3(grid), dim3(threads), a.lds_total, st, a);
        return;
    }
    if (a.use_fx2) {
        if (fixup) hipLaunchKernelGGL((k_parser_reg<true, false, 3>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else if (threads <= 768) hipLaunchKernelGGL((k_parser_reg<false, false, 3, 768>), dim3(grid), dim3(threads), a.lds_total, st, a);
        else hipLaunchKernelGGL((k_parser_reg<false, false, 3>), dim3(grid), dim3(threads), a.lds_total, st, a);
        return;
    }
    if (fixup) hipLaunchKernelGGL((k_parser_reg<true, false>), dim3(grid), dim3(threads), a.lds_total, st, a);
    else if (a.stage_nbuf) hipLaunchKernelGGL((k_parser_reg<false, true>), dim3(grid), dim3(threads), a.lds_total, st, a);
    else hipLaunchKernelGGL((k_parser_reg<false, false>), dim3(grid), dim3(threads), a.lds_total, st, a);
}

void launch_parser_tile(const ParserMatchArgs &a, int grid, int threads, hipStream_t st) {
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        (void) hipFuncSetAttribute((const void *) k_parser_tile, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(k_parser_tile, dim3(grid), dim3(threads), a.lds_total, st, a);
}
