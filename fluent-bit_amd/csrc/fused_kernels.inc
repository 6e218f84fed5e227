// fused_kernels.inc -- flb_filter_do over [filter_parser, filter_grep] without the parsed chunk.
//
// The unfused chain writes every parsed record (k_parser_emit), decodes the parsed chunk again for the rules
// (k_grep_match) and copies the kept records (k_gather).  What the engine can observe of the pair is only
// grep's output and the per-filter record / byte counts flb_filter_do feeds its metrics with
// (src/flb_filter.c:213-222,272-312).  So after filter_parser's pass 1 (locate / rx / finish: spans, timestamps
// and sizes of every record in HBM columns):
//
//   k_pg_decide  one record per lane, coalesced column reads: grep's rules evaluated on the record filter_parser
//                WOULD emit -- for a parsed record its body map is the kept named fields in order, every value a
//                STR, so a rule's key names a capture span (grep.c:167-194,250-284; flb_ra_key.c:118: the LAST
//                entry of that name; :418-420: STR values only) and the match-only DFA runs on the span's bytes;
//                an unparsed record's body is the canonical re-pack of the original map, same keys and value
//                types, so the rules run on the original bytes.  keep_len[r] = the parsed record's size when kept
//   k_scan_*     keep_len -> output offsets
//   k_pg_emit    filter_parser's write_record for the kept records only, straight to their offsets; a wave compacts
//                the kept rows of its block into an LDS queue first so that its lanes stay busy
//
// (A single kernel doing locate + capture program + fields + rules per lane was built and measured first: with
// the phases inlined it spills inside the byte loop of the capture program, with the phases out of line the
// call-boundary spills cost more than the column round trips save -- 3.9 ms against 2.9 ms per 4 M records.)

__global__ void __launch_bounds__(256) k_pg_decide(PgDecideArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    // the rules' match-only DFAs (byte classes, transitions, final flags) into LDS: a few hundred bytes each for
    // the usual patterns, touched once per byte of every tested field
    LDS_AS uint8_t *lds = (LDS_AS uint8_t *) g_lds;
    for (int i = 0; i < a.nrules; i++) {
        if (a.rule_lds_off[i] == 0xFFFFFFFFu) continue;
        const uint8_t *src = a.rules[i].dfa.cls;
        for (uint32_t k = threadIdx.x; k < a.rule_lds_bytes[i]; k += blockDim.x) lds[a.rule_lds_off[i] + k] = src[k];
    }
    __syncthreads();
    const uint64_t n = a.n, nc = a.n_cols;
    uint32_t n_out = 0, n_keep = 0;
    unsigned long long out_bytes = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t) gridDim.x * blockDim.x) {
        // rows the inline evaluation (k_parser_rx + k_parser_finish) has settled keep their keep_len
        if (a.keep_len[r] != PG_UNDECIDED) continue;
        uint32_t keep_len = 0;
        // everything the decision needs from the columns, loaded together (one round trip, not five)
        const uint32_t out_len = a.out_len[r], flags = a.info[r], drop_m = a.info[12 * nc + r], val_off = a.info[1 * nc + r];
        const uint64_t roff = a.row_off[r];
        if (out_len) {
            n_out++;
            out_bytes += out_len;
            const uint8_t *rec = a.data + roff;
            bool keep;
            if (flags & RF_PARSED) {
                // (a parsed time that reads as a group marker to filter_grep's decoder: tile_kernels.inc k_parser_reg)
                if (a.info[4 * nc + r] >= 0xfffffffeu) atomicAdd(&a.counts[MW_TIME_MARKER], 1ull);
                CapsView cv;
                cv.base = a.caps; cv.n = nc; cv.r = r;
                keep = pg_grep_parsed(a.rules, a.nrules, a.logical_op, a.rule_fmask, a.rule_lds_off, drop_m, rec + val_off, cv, lds);
            }
            else {
                // unparsed: the canonical re-pack of the original body -- same keys, same value types
                GrepArgs ga;
                ga.rules = a.rules; ga.nrules = a.nrules; ga.logical_op = a.logical_op; ga.nslots = 0; ga.host_collect = 0;
                Event ev;
                ev.body = rec + a.info[6 * nc + r]; ev.body_end = ev.body + a.info[7 * nc + r];
                bool valid = false;
                keep = grep_decide(ga, ev, &valid);
            }
            if (keep) { keep_len = out_len; n_keep++; }
        }
        a.keep_len[r] = keep_len;
    }
    // one set of atomics per wave (same-address atomics serialise at ~12 ns each: the grid is kept small)
    for (int o = 32; o > 0; o >>= 1) {
        n_out += __shfl_down(n_out, o, 64); n_keep += __shfl_down(n_keep, o, 64); out_bytes += __shfl_down(out_bytes, o, 64);
    }
    if (lane == 0) {
        if (out_bytes) atomicAdd(&a.counts[MW_PG_BYTES], out_bytes);
        if (n_keep) atomicAdd(&a.counts[MW_PG_KEEP], (unsigned long long) n_keep);
        if (n_out) atomicAdd(&a.counts[MW_PG_OUT], (unsigned long long) n_out);
    }
}

// The kept records written by filter_parser's write_record.  A wave owns PGE_ROWS consecutive rows: it reads their lengths
// (eight loads in flight), compacts the indices of the kept ones into an LDS queue in row order (ballot + prefix count, no
// global atomics) and then takes the queued records 64 at a time -- consecutive kept rows are consecutive in the output,
// so each lane writes its record into the wave's LDS staging area at the record's offset inside that range and the wave
// flushes the range with coalesced 16 B / lane stores (a lane writing its 275 bytes straight to global memory costs a
// sector write per 16-byte store: 6x the bytes on the HBM side).  A record's fields come from its descriptor (rows the
// single pass kept: RF_DESC) or from the record / span columns (rows k_pg_decide settled).
// The time text at byte `at` of the chunk through the parser's compiled plan (kdev.inc time_fast_compiled; the plan's 32 dwords sit behind
// the parser's pair tables in device memory, where k_parser_reg stages them from).  Out of line: inlined, its registers came on top of
// write_record's and the kernel lost half its waves (260 registers; 0.55 -> 0.97 ms per 1 M kept records).
__device__ __noinline__ bool pge_time(const uint8_t *data, uint64_t bytes, uint64_t at, const DevParser *ps, int64_t *sec) {
    const uint32_t *cp = (const uint32_t *) (ps->fx2.base + (ps->fx2.bytes - 128u));
    if (!ps->fx2.ok || cp[31] == 0) return false;
    const uint8_t *tp = data + at;
    const uint64_t left = bytes - at;                    // (32 bytes from the text's start: inside the chunk except for its last records)
    const v4u32 t0 = left >= 32 ? ldu128(tp) : load16(tp, 0, (uint32_t) left), t1 = left >= 32 ? ldu128(tp + 16) : load16(tp + 16, 0, left > 16 ? (uint32_t) left - 16 : 0);
    const uint32_t tw[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    int64_t s2 = 0;
    const bool ok = time_fast_compiled(cp, ps->time_with_tz, ps->time_offset, tw, &s2);
    *sec = s2;
    return ok;
}
// PLAIN (round 5): the build for what the single pass leaves behind on ordinary data -- every kept record with its descriptor, the
// parser's fields plain strings (EmitCfg::ok) -- WITHOUT the general writer in it: write_record (Types casts, reserved keys, decoders'
// rows, records larger than the staging area) made the kernel 254 registers wide, two waves per SIMD, for code the benchmark never
// runs.  A record the plain build does not take is counted (counts[MW_PG_LEFT]) and left alone; the host then runs the general build over the
// chunk (same bytes for the records both write).  Its staging area is a little smaller so that three workgroups share a CU's LDS.
constexpr int PGE_ROWS = 512;
constexpr int PGE_STG_GENERAL = 9728;        // staging bytes per wave (about 34 records of 275 B)
constexpr int PGE_STG_PLAIN = 8192;
template <bool PLAIN>
__global__ void __launch_bounds__(256) k_pg_emit(PgEmitArgs a) {
    constexpr int PGE_STG = PLAIN ? PGE_STG_PLAIN : PGE_STG_GENERAL;
    if (a.out_cap && a.out_off[a.n] > a.out_cap) return;            // (ParserEmitArgs::out_cap)
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ncap = 2 * (uint32_t) a.parsers[0].nfields;
    // dynamic LDS: per wave [queue PGE_ROWS u32][spans ncap x 64 u16][staging PGE_STG]
    const uint32_t per_wave = PGE_ROWS * 4 + ((ncap * 128 + 15) & ~15u) + PGE_STG;
    LDS_AS uint8_t *wb = (LDS_AS uint8_t *) g_lds + (size_t) wave * per_wave;
    LDS_AS uint32_t *q = (LDS_AS uint32_t *) wb;
    LDS_AS uint16_t *spans = (LDS_AS uint16_t *) (wb + PGE_ROWS * 4);
    LDS_AS uint8_t *stg = wb + PGE_ROWS * 4 + ((ncap * 128 + 15) & ~15u);
    const uint64_t wave_id = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    for (uint64_t base = wave_id * PGE_ROWS; base < a.n; base += nwaves * PGE_ROWS) {
        uint32_t kl[PGE_ROWS / 64];
        #pragma unroll
        for (uint32_t j = 0; j < PGE_ROWS / 64; j++) { const uint64_t r = base + 64 * j + lane; kl[j] = r < a.n ? a.keep_len[r] : 0; }
        uint32_t cnt = 0;
        #pragma unroll
        for (uint32_t j = 0; j < PGE_ROWS / 64; j++) {
            const bool kept = kl[j] != 0;
            const uint64_t km = __ballot(kept);
            if (kept) q[cnt + (uint32_t) __builtin_popcountll(km & ((1ull << lane) - 1))] = 64 * j + lane;
            cnt += (uint32_t) __builtin_popcountll(km);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
            const uint32_t nk = cnt - k0 < 64 ? cnt - k0 : 64;
            const bool actv = lane < nk;
            uint64_t r = 0, o0 = 0, o1 = 0, roff = 0, roff1 = 0;
            uint32_t fl = 0;
            if (actv) {
                r = base + q[k0 + lane];
                o0 = a.out_off[r]; o1 = a.out_off[r + 1]; roff = a.row_off[r]; roff1 = a.row_off[r + 1]; fl = a.info[r];
            }
            RecInfo ri;
            recinfo_init(ri);
            uint64_t nm = 0;
            if (actv) {
                if ((fl & RF_DESC) && a.desc) {
                    const uint32_t *dp = a.desc + r * a.dstride;
                    const v4u32 d0 = *(const v4u32 *) dp, d1 = *(const v4u32 *) (dp + 4);
                    ri.flags = fl; ri.ts_sec = d0.x; ri.ts_nsec = d0.y; ri.val_off = d0.z; ri.drop_mask = d0.w;
                    ri.meta_off = d1.x; ri.meta_len = d1.y; ri.nkept = d1.z; ri.parser_idx = 0; ri.val_len = 0;
                    spans[0 * 64 + lane] = (uint16_t) (d1.w & 0xFFFF);
                    if (ncap > 1) spans[1 * 64 + lane] = (uint16_t) (d1.w >> 16);
                    for (uint32_t c = 2; c < ncap; c += 8) {
                        const v4u32 dv = *(const v4u32 *) (dp + 8 + (c - 2) / 2);
                        const uint32_t wv[4] = {dv.x, dv.y, dv.z, dv.w};
                        #pragma unroll
                        for (uint32_t j = 0; j < 4; j++) {
                            if (c + 2 * j < ncap) spans[(c + 2 * j) * 64 + lane] = (uint16_t) (wv[j] & 0xFFFF);
                            if (c + 2 * j + 1 < ncap) spans[(c + 2 * j + 1) * 64 + lane] = (uint16_t) (wv[j] >> 16);
                        }
                    }
                    if (fl & RF_TIMEPEND) {
                        // The single pass left this record's time lookup to the records grep keeps (TileCfg::defer_time): the text has the
                        // plan's length and an in-range year, the descriptor carries the event's own time.  A text the fixed-layout plan does
                        // not settle, or a time the encoder refuses, is reported: the host repeats the call with the lookup in the single pass.
                        const DevParser &ps = a.parsers[0];
                        const uint32_t tb = spans[(2 * (uint32_t) ps.time_field) * 64 + lane];
                        int64_t tsec = ri.ts_sec, tnsec = ri.ts_nsec;
                        int64_t s2 = 0;
                        const bool tok = pge_time(a.data, a.bytes, roff + ri.val_off + tb, &ps, &s2);
                        if (tok && s2 != 0) { tsec = s2; tnsec = 0; }
                        if (!tok || encoder_refuses_time(tsec, tnsec)) atomicAdd(&a.counts[MW_PG_TIME_FAIL], 1ull);
                        else { ri.ts_sec = (uint32_t) tsec; ri.ts_nsec = (uint32_t) tnsec; }
                    }
                }
                else if constexpr (!PLAIN) {
                    ri = rec_load(a.info, a.n_cols, r);
                    nm = a.null_mask[r];
                    if (ri.val_len < 0xFFFF && (ri.flags & RF_PARSED)) spans_to_lds(a.caps, a.n_cols, r, ncap, spans + lane, 64);
                }
            }
            const bool lds_caps = actv && (ri.flags & RF_PARSED) && ((fl & RF_DESC) || ri.val_len < 0xFFFF);
            // ---- batches of consecutive queued records whose output fits the staging area
            uint32_t lo = 0;
            while (lo < nk) {
                const uint64_t batch_base = __shfl(o0, (int) lo, 64);
                const uint32_t align = (uint32_t) (batch_base & 15);
                const bool fit = lane >= lo && lane < nk && (o1 - batch_base + align) <= (uint64_t) PGE_STG;
                const uint64_t mask = __ballot(fit) >> lo;
                uint32_t m = (~mask == 0) ? 64 - lo : (uint32_t) __builtin_ctzll(~mask);
                if (m > nk - lo) m = nk - lo;
                const bool direct = m == 0;                  // one record larger than the staging area: straight to global memory
                if (direct) m = 1;
                if constexpr (PLAIN) {
                    if (lane >= lo && lane < lo + m && o1 > o0) {
                        if (direct || !(lds_caps && a.ec.ok && ri.parser_idx == 0 && (fl & RF_DESC))) atomicAdd(&a.counts[MW_PG_LEFT], 1ull);   // the general build's
                        else {
                            CapsLdsView cv;
                            cv.col = spans + lane; cv.stride = 64;
                            cv.base = a.caps; cv.n = a.n_cols; cv.r = r;
                            LdsSink sk(stg + align + (uint32_t) (o0 - batch_base));
                            sk.src_end = a.data + a.bytes;
                            sk.limit = sk.p + (uint32_t) (o1 - o0);
                            write_record_plain(sk, a.ec, a.data + roff, ri, cv);
                        }
                    }
                }
                else
                if (lane >= lo && lane < lo + m && o1 > o0) {
                    CapsLdsView cv;
                    cv.col = spans + lane; cv.stride = 64;
                    cv.base = a.caps; cv.n = a.n_cols; cv.r = r;
                    CapsView cg;
                    cg.base = a.caps; cg.n = a.n_cols; cg.r = r;
                    if (direct) {
                        ByteSink sk(a.out + o0);
                        sk.limit = a.out + o1;
                        if (lds_caps) write_record(sk, a.cfg, a.parsers, a.data + roff, a.data + roff1, ri, cv, nm);
                        else write_record(sk, a.cfg, a.parsers, a.data + roff, a.data + roff1, ri, cg, nm);
                    }
                    else {
                        LdsSink sk(stg + align + (uint32_t) (o0 - batch_base));
                        sk.src_end = a.data + a.bytes;
                        sk.limit = sk.p + (uint32_t) (o1 - o0);
                        if (lds_caps && a.ec.ok && ri.parser_idx == 0) write_record_plain(sk, a.ec, a.data + roff, ri, cv);
                        else if (lds_caps) write_record(sk, a.cfg, a.parsers, a.data + roff, a.data + roff1, ri, cv, nm);
                        else write_record(sk, a.cfg, a.parsers, a.data + roff, a.data + roff1, ri, cg, nm);
                    }
                }
                if (!direct) {
                    const uint32_t total = (uint32_t) (__shfl(o1, (int) (lo + m - 1), 64) - batch_base);
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");     // staged bytes visible to the wave
                    uint8_t *dst = a.out + (batch_base - align);               // 16 B aligned
                    const uint32_t n16 = (align + total + 15) / 16;
                    for (uint32_t u = lane; u < n16; u += 64) {
                        const uint32_t b0 = u * 16, b1 = b0 + 16;
                        if (b0 >= align && b1 <= align + total) *(v4u32 *) (dst + b0) = *(LDS_AS v4u32 *) (stg + b0);
                        else {
                            const uint32_t s0 = b0 < align ? align : b0, s1 = b1 > align + total ? align + total : b1;
                            for (uint32_t qq = s0; qq < s1; qq++) dst[qq] = stg[qq];
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");     // staging area reusable
                }
                lo += m;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
}

void launch_pg_decide(const PgDecideArgs &a, int cus, hipStream_t st) {
    if (a.n == 0) return;
    uint64_t blocks = (a.n + 255) / 256, cap = (uint64_t) cus * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_pg_decide, dim3((unsigned) blocks), dim3(256), a.lds_total, st, a);
}
static void launch_pg_emit_t(const PgEmitArgs &a, int nfields, int cus, hipStream_t st, bool plain) {
    if (a.n == 0) return;
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        (void) hipFuncSetAttribute((const void *) k_pg_emit<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void) hipFuncSetAttribute((const void *) k_pg_emit<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    const uint32_t ncap = 2 * (uint32_t) nfields;
    const size_t lds = (size_t) 4 * (PGE_ROWS * 4 + ((ncap * 128 + 15) & ~15u) + (plain ? PGE_STG_PLAIN : PGE_STG_GENERAL));
    uint64_t blocks = (a.n + 4 * PGE_ROWS - 1) / (4 * PGE_ROWS), cap = (uint64_t) cus * (plain ? 12 : 8);
    if (blocks > cap) blocks = cap;
    if (plain) hipLaunchKernelGGL(k_pg_emit<true>, dim3((unsigned) blocks), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(k_pg_emit<false>, dim3((unsigned) blocks), dim3(256), lds, st, a);
}
void launch_pg_emit(const PgEmitArgs &a, int nfields, int cus, hipStream_t st) { launch_pg_emit_t(a, nfields, cus, st, false); }
void launch_pg_emit_plain(const PgEmitArgs &a, int nfields, int cus, hipStream_t st) { launch_pg_emit_t(a, nfields, cus, st, true); }
