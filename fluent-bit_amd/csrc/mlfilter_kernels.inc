// mlfilter_kernels.inc -- filter_multiline, mode parser with buffer off (plugins/filter_multiline/ml.c:839-909): flb_ml_append_event /
// flb_ml_append_object (src/multiline/flb_ml.c:763-875, process_append / package_content :207-501) and flb_ml_flush_stream_group
// (:1590-1800) for the records of one chunk, around the multiline core of ml_kernels.inc.
//   k_mlf_class   a lane per row: does the decoder hand the row out (not a group marker, not an empty row), the first row it refuses,
//                 rows with a non-empty metadata map
//   k_mlf_items   a lane per row that is handed out: item k = its text (the first entry whose key is a STR equal to key_content and
//                 whose value is a STR: get_key_id), its time, its class
//   [k_ml_match]
//   k_mlf_fix     an item that is not processed: no rule matches it, its transition is the identity, it leaves alone and breaks the
//                 group in front of it (ENDSWITH / EQ: it and the item in front of it flush)
//   [k_ml_fscan_*, k_ml_act, scans, k_ml_ghead, k_ml_trunc / k_ml_override]
//   k_mlf_plan    which items register a time and a first-line map (flb_ml_register_context) and when: in front of their own flush or
//                 behind it -- an item whose rule flushes the group registers ITSELF into the emptied group (package_content :271-273)
//   k_mlf_size    the first item of a group sizes the group's record, k_mlf_emit writes it: ONE function, mlf_record, behind a counting
//                 sink and behind a sink bounded by the record's own room; every item copies its own text to its place
// Included inside namespace flbgpu after kdev.inc and lane_rows.inc.

constexpr int MLF_BLOCK = 256;
enum { MLF_ALONE = 0, MLF_START = 1, MLF_CONT = 2, MLF_APP = 3 };

struct MlfCount {
    uint64_t n = 0;
    DEV void put(uint32_t) { n++; }
    DEV void copy(const uint8_t *, uint32_t len) { n += len; }
    DEV void skip(uint64_t len) { n += len; }
    DEV uint64_t pos() const { return n; }
};
// [base, limit) is the room: nothing is stored at or past limit, p keeps counting
struct MlfSink {
    uint8_t *base, *p, *limit;
    bool over = false;
    DEV MlfSink(uint8_t *dst, uint8_t *lim) : base(dst), p(dst), limit(lim) {}
    DEV void put(uint32_t b) {
        if (p < limit) *p = (uint8_t) b; else over = true;
        p++;
    }
    DEV void copy(const uint8_t *src, uint32_t len) {
        const uint64_t room = p < limit ? (uint64_t) (limit - p) : 0;
        const uint32_t n = room < len ? (uint32_t) room : len;
        ByteSink bs(p);
        bs.copy(src, n);
        if (n < len) over = true;
        p += len;
    }
    DEV void skip(uint64_t len) { p += len; if (p > limit) over = true; }
    DEV uint64_t pos() const { return (uint64_t) (p - base); }
};

struct MlfIt { uint32_t cat; bool trunc, ba; };
DEV MlfIt mlf_it(const MlfArgs &a, uint64_t k) {
    MlfIt it;
    const uint32_t act = a.act[k];
    if (a.cls[k] == MLF_NOTPROC) { it.cat = MLF_ALONE; it.trunc = false; it.ba = true; return it; }
    if (!a.regex) { it.cat = MLF_APP; it.trunc = false; it.ba = (act & MLK_BA) != 0; return it; }
    const uint32_t kk = act & MLK_MASK;
    it.cat = kk == MLK_START ? (uint32_t) MLF_START : kk == MLK_CONT ? (uint32_t) MLF_CONT : (uint32_t) MLF_ALONE;
    // (a line nobody takes is never cut: flb_ml_rule_process answers -1 before anything is concatenated)
    it.trunc = it.cat != MLF_ALONE && (act & MLK_TRUNC);
    it.ba = it.cat == MLF_ALONE || (act & MLK_BA);
    return it;
}
// the group of item k >= 1: its first and last record (item 0, the empty carried buffer, is nobody's first)
DEV void mlf_group(const MlfArgs &a, uint64_t k, uint64_t &f, uint64_t &L) {
    const uint64_t g = a.gidx[k] + a.head[k] - 1;
    f = a.ghead[g];
    if (f == 0) f = 1;
    L = a.ghead[g + 1] - 1;
}
// after item k the group is empty and holds k's own map and time
DEV bool mlf_seeding(const MlfArgs &a, uint64_t k) {
    if (k == 0 || !a.regex) return false;
    const MlfIt it = mlf_it(a, k);
    return (it.cat == MLF_START || it.cat == MLF_CONT) && !it.trunc && it.ba;
}
DEV bool mlf_has_seed(const MlfArgs &a, uint64_t f) { return f >= 2 && mlf_seeding(a, f - 1); }
// item k (of the group that starts at f) registers its time and map in front of its own flush
DEV bool mlf_pre_reg(const MlfArgs &a, uint64_t k, uint64_t f) {
    const MlfIt it = mlf_it(a, k);
    if (it.cat == MLF_ALONE) return true;
    if (it.cat == MLF_APP) return k == f;
    if (it.trunc) return false;
    if (it.cat == MLF_START) return true;
    if (it.ba) return false;                       // the flush comes first (try_flushing_buffer), the registration behind it
    if (mlf_has_seed(a, f)) return false;
    if (k == f) return true;
    if (k == f + 1) { const MlfIt h = mlf_it(a, f); return h.cat == MLF_START && h.trunc; }
    return false;
}

// bytes of item k's own text that enter its group's buffer, with the separator in front
template <class S> DEV void mlf_piece(S &s, const MlfArgs &a, uint64_t k) {
    const MlfIt it = mlf_it(a, k);
    if (it.cat == MLF_ALONE) return;
    const uint32_t act = a.act[k], c = a.c[k], sep = (a.regex && (act & MLK_SEP)) ? 1u : 0u;
    if (sep) s.put('\n');
    if (it.cat == MLF_CONT && a.ll[k] == 0) { s.put('\n'); return; }
    s.copy(a.data + a.ls[k], c - sep);
}

template <class S> DEV void mlf_head(S &s, uint32_t sec, uint32_t nsec, bool trunc) {
    s.put(0x92); s.put(0x92); s.put(0xd7); s.put(0x00);
    pk_be(s, sec, 4); pk_be(s, nsec, 4);
    s.put(0xdf); pk_be(s, trunc ? 1u : 0u, 4);               // the encoder's metadata map32
    if (trunc) {
        const char *m = "multiline_truncated";
        s.put(0xb3);
        for (int i = 0; i < 19; i++) s.put((uint8_t) m[i]);
        s.put(0xc3);
    }
}

// the time registered last in front of slot `upto` (exclusive)
DEV void mlf_time(const MlfArgs &a, uint64_t upto, uint32_t &sec, uint32_t &nsec) {
    const uint64_t cnt = a.evoff[upto];
    if (cnt == 0) { sec = a.carry_sec; nsec = a.carry_nsec; return; }
    const uint64_t k = a.regidx[cnt - 1] >> 1;
    sec = a.tsec[k]; nsec = a.tnsec[k];
}

// item k's whole map again (msgpack_pack_object): a record that is not processed, a group whose buffer is empty, a seed nobody joined
template <class S> DEV bool mlf_whole(S &s, const MlfArgs &a, uint64_t k, uint32_t sec, uint32_t nsec) {
    const uint64_t r = a.irow[k];
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    const Event ev = decode_event(rec, end);
    if ((ev.flags & (RF_BAD | RF_SKIP)) || ev.body_end != end) return false;
    mlf_head(s, sec, nsec, false);
    return mp_canon(ev.body, end, s, 1) == end;
}

// the record of the group [f, L] (flb_ml_flush_stream_group): *slot = where the concatenation starts inside it (MLF_NOSLOT: nowhere)
template <class S> DEV bool mlf_record(S &s, const MlfArgs &a, uint64_t f, uint64_t L, uint32_t *slot) {
    *slot = MLF_NOSLOT;
    const MlfIt hf = mlf_it(a, f);
    uint32_t sec, nsec;
    mlf_time(a, 2 * L + 1, sec, nsec);
    if (hf.cat == MLF_ALONE) return mlf_whole(s, a, f, sec, nsec);
    const uint64_t C = a.coff[L + 1] - a.coff[f];
    // whose map: the seed's, else the first item that registers in front of the flush
    uint64_t owner = 0;
    if (mlf_has_seed(a, f)) owner = f - 1;
    else if (mlf_pre_reg(a, f, f)) owner = f;
    else if (f + 1 <= L && mlf_pre_reg(a, f + 1, f)) owner = f + 1;
    if (owner && C == 0) return mlf_whole(s, a, owner, sec, nsec);
    const bool trunc = hf.trunc || mlf_it(a, L).trunc;
    mlf_head(s, sec, nsec, trunc);
    if (!owner) {
        // no first-line map: {key_content: buffer}
        s.put(0x81);
        pk_str_hdr(s, a.key_len);
        for (uint32_t i = 0; i < a.key_len; i++) s.put(a.key[i]);
        pk_str_hdr(s, (uint32_t) C);
        *slot = (uint32_t) s.pos();
        s.skip(C);
        return true;
    }
    const uint64_t r = a.irow[owner];
    const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
    const Event ev = decode_event(rec, end);
    if ((ev.flags & (RF_BAD | RF_SKIP)) || ev.body_end != end) return false;
    const Tok m = mp_tok(ev.body, end);
    if (m.type != T_MAP) return false;
    pk_map_hdr(s, m.len);
    const uint8_t *p = m.next;
    uint64_t len = a.key_len;                       // the reference's `len`: key_content's length until the first replacement, then the buffer's
    for (uint32_t i = 0; i < m.len; i++) {
        const Tok kt = mp_tok(p, end);
        const uint8_t *kend = mp_end_of(kt, p, end, 2);
        if (!kend) return false;
        const uint8_t *vend = mp_skip(kend, end, 2);
        if (!vend) return false;
        bool hit = kt.type == T_STR && kt.len == len;
        for (uint64_t j = 0; hit && j < len; j++) {         // strncmp(key, key_content, len)
            const uint32_t x = ld8(kt.next + j), y = j < a.key_len ? a.key[j] : 0u;
            if (x != y) hit = false;
            else if (x == 0) break;
        }
        if (!mp_canon(p, end, s, 2)) return false;
        if (hit) {
            pk_str_hdr(s, (uint32_t) C);
            if (*slot == MLF_NOSLOT) { *slot = (uint32_t) s.pos(); s.skip(C); }
            else for (uint64_t k = f; k <= L; k++) mlf_piece(s, a, k);
            len = C;
        }
        else if (!mp_canon(kend, end, s, 2)) return false;
        p = vend;
    }
    return p == end;
}

__global__ void __launch_bounds__(MLF_BLOCK) k_mlf_class(MlfArgs a) {
    unsigned long long n_meta = 0;
    for (uint64_t r = (uint64_t) blockIdx.x * MLF_BLOCK + threadIdx.x; r < a.n; r += (uint64_t) gridDim.x * MLF_BLOCK) {
        const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
        uint32_t keep = 0;
        if (rec != end) {
            const Event ev = decode_event(rec, end);
            if ((ev.flags & RF_BAD) || ev.body_end != end) atomicMin(&a.w->first_bad, (unsigned long long) r);
            else if (!(ev.flags & RF_SKIP)) {
                keep = 1;
                if (ev.meta) { const Tok mt = mp_tok(ev.meta, end); if (mt.type == T_MAP && mt.len > 0) n_meta++; }
            }
        }
        a.keep[r] = keep;
    }
    n_meta = lane_wave_sum(n_meta);
    if ((threadIdx.x & 63u) == 0 && n_meta) atomicAdd(&a.w->meta_refused, n_meta);
}

__global__ void __launch_bounds__(MLF_BLOCK) k_mlf_items(MlfArgs a) {
    __shared__ uint8_t s_key[256];
    for (uint32_t i = threadIdx.x; i < a.key_len && i < 256; i += MLF_BLOCK) s_key[i] = a.key[i];
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.ls[0] = 0; a.ll[0] = 0; a.irow[0] = 0; a.cls[0] = MLF_RULES; a.tsec[0] = 0; a.tnsec[0] = 0; }
    for (uint64_t r = (uint64_t) blockIdx.x * MLF_BLOCK + threadIdx.x; r < a.n; r += (uint64_t) gridDim.x * MLF_BLOCK) {
        if (!a.keep[r]) continue;
        const uint64_t k = a.koff[r] + 1;
        if (k >= a.N) continue;
        const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
        const Event ev = decode_event(rec, end);
        uint64_t ls = 0;
        uint32_t ll = 0, cls = MLF_NOTPROC;
        if (!(ev.flags & (RF_BAD | RF_SKIP)) && a.has_key) {
            const Tok m = mp_tok(ev.body, end);
            const uint8_t *p = m.next;
            for (uint32_t i = 0; m.type == T_MAP && i < m.len; i++) {
                const Tok kt = mp_tok(p, end);
                const uint8_t *kend = mp_end_of(kt, p, end, 2);
                if (!kend) break;
                const Tok vt = mp_tok(kend, end);
                const uint8_t *vend = mp_end_of(vt, kend, end, 2);
                if (!vend) break;
                if (kt.type == T_STR && vt.type == T_STR && kt.len == a.key_len) {
                    bool eq = true;
                    for (uint32_t j = 0; eq && j < kt.len; j++) eq = ld8(kt.next + j) == s_key[j];
                    if (eq) { ls = (uint64_t) (vt.next - a.data); ll = vt.len; cls = MLF_RULES; break; }
                }
                p = vend;
            }
        }
        // an ENDSWITH text shorter than the string is not processed (package_content :279)
        if (cls == MLF_RULES && a.type == ML_ENDSWITH && a.match_len > ll) cls = MLF_NOTPROC;
        if (cls == MLF_NOTPROC) { ls = 0; ll = 0; }
        a.ls[k] = ls; a.ll[k] = ll; a.irow[k] = (uint32_t) r; a.cls[k] = (uint8_t) cls;
        a.tsec[k] = (uint32_t) (uint64_t) ev.sec; a.tnsec[k] = (uint32_t) (uint64_t) ev.nsec;
    }
}

__global__ void __launch_bounds__(MLF_BLOCK) k_mlf_fix(MlfArgs a) {
    for (uint64_t k = (uint64_t) blockIdx.x * MLF_BLOCK + threadIdx.x; k < a.N; k += (uint64_t) gridDim.x * MLF_BLOCK) {
        if (k == 0) continue;
        const bool np = a.cls[k] == MLF_NOTPROC;
        if (a.regex) {
            if (np) { a.info[k] = 0; a.F[k] = 0xFEDCBA9876543210ull; }
        }
        else {
            // ENDSWITH / EQ: bit 0 of info flushes behind the item; bit 1 (dropped) is never set here.  F is left as k_ml_match wrote it: its
            // guess of the group's head re-matches the text of item k - 1 and knows nothing of a not-processed neighbour, so the "how the
            // buffer ends" component is wrong around such items.  Nothing reads it: it only decides the separator, and with key_content
            // set (has_key_content = 1, run_mlfilter_dev) breakline_prepare adds none.  This is relied upon.
            uint32_t info = a.info[k] & ~2u;
            if (np) info = 1;
            else if (k + 1 < a.N && a.cls[k + 1] == MLF_NOTPROC) info |= 1u;
            a.info[k] = info;
        }
    }
}

__global__ void __launch_bounds__(MLF_BLOCK) k_mlf_plan(MlfArgs a) {
    unsigned long long n_trunc = 0, n_empty = 0;
    for (uint64_t k = (uint64_t) blockIdx.x * MLF_BLOCK + threadIdx.x; k < a.N; k += (uint64_t) gridDim.x * MLF_BLOCK) {
        uint32_t e0 = 0, e1 = 0;
        if (k > 0) {
            uint64_t f, L;
            mlf_group(a, k, f, L);
            const MlfIt it = mlf_it(a, k);
            e0 = mlf_pre_reg(a, k, f) ? 1u : 0u;
            e1 = mlf_seeding(a, k) ? 1u : 0u;
            if (it.trunc) n_trunc++;
            if (it.cat == MLF_START && a.ll[k] == 0) n_empty++;
        }
        a.ev[2 * k] = e0; a.ev[2 * k + 1] = e1;
    }
    n_trunc = lane_wave_sum(n_trunc); n_empty = lane_wave_sum(n_empty);
    if ((threadIdx.x & 63u) == 0) {
        if (n_trunc) atomicAdd(&a.w->truncated, n_trunc);
        if (n_empty) atomicAdd(&a.w->empty_start, n_empty);
    }
}

__global__ void __launch_bounds__(MLF_BLOCK) k_mlf_regidx(MlfArgs a) {
    for (uint64_t s = (uint64_t) blockIdx.x * MLF_BLOCK + threadIdx.x; s < 2 * a.N; s += (uint64_t) gridDim.x * MLF_BLOCK)
        if (a.ev[s]) a.regidx[a.evoff[s]] = (uint32_t) s;
}

// a seed nobody joins leaves with its own map: the next record leaves alone, or the call ends
DEV bool mlf_dups(const MlfArgs &a, uint64_t k) {
    if (!mlf_seeding(a, k)) return false;
    return k + 1 == a.N || mlf_it(a, k + 1).cat == MLF_ALONE;
}

__global__ void __launch_bounds__(MLF_BLOCK) k_mlf_size(MlfArgs a) {
    unsigned long long n_big = 0, n_mis = 0;
    for (uint64_t k = (uint64_t) blockIdx.x * MLF_BLOCK + threadIdx.x; k < a.N; k += (uint64_t) gridDim.x * MLF_BLOCK) {
        uint32_t plen = 0, pre = MLF_NOSLOT, dup = 0, nrec = 0;
        if (k > 0) {
            uint64_t f, L;
            mlf_group(a, k, f, L);
            if (k == f) {
                MlfCount cs;
                if (!mlf_record(cs, a, f, L, &pre)) n_mis++;
                if (cs.n > 0xFFFFFF00ull) { n_big++; cs.n = 0; }
                plen = (uint32_t) cs.n; nrec = 1;
            }
            if (mlf_dups(a, k)) {
                MlfCount cs;
                if (!mlf_whole(cs, a, k, 0, 0)) n_mis++;
                if (cs.n + plen > 0xFFFFFF00ull) { n_big++; cs.n = 0; }
                dup = (uint32_t) cs.n; plen += dup; nrec++;
            }
            if (k == a.N - 1) {
                const uint64_t cnt = a.evoff[2 * a.N];
                a.w->has_reg = cnt ? 1u : 0u;
                if (cnt) { const uint64_t q = a.regidx[cnt - 1] >> 1; a.w->last_sec = a.tsec[q]; a.w->last_nsec = a.tnsec[q]; }
            }
        }
        a.plen[k] = plen; a.pre[k] = pre; a.dup[k] = dup; a.nrec[k] = nrec;
    }
    n_big = lane_wave_sum(n_big); n_mis = lane_wave_sum(n_mis);
    if ((threadIdx.x & 63u) == 0) {
        if (n_big) atomicAdd(&a.w->big, n_big);
        if (n_mis) atomicAdd(&a.w->mismatch, n_mis);
    }
}

__global__ void __launch_bounds__(MLF_BLOCK) k_mlf_emit(MlfArgs a) {
    unsigned long long n_mis = 0;
    for (uint64_t k = (uint64_t) blockIdx.x * MLF_BLOCK + threadIdx.x; k < a.N; k += (uint64_t) gridDim.x * MLF_BLOCK) {
        if (k == 0) { a.rows_out[a.ridx[a.N]] = a.po[a.N]; continue; }
        uint64_t f, L;
        mlf_group(a, k, f, L);
        const uint32_t dup = a.dup[k];
        if (k == f) {
            const uint64_t room = a.plen[k] - dup;
            MlfSink s(a.out + a.po[k], a.out + a.po[k] + room);
            uint32_t slot;
            if (!mlf_record(s, a, f, L, &slot) || s.over || s.pos() != room || slot != a.pre[k]) n_mis++;
            a.rows_out[a.ridx[k]] = a.po[k];
        }
        const uint32_t pre = a.pre[f];
        if (pre != MLF_NOSLOT && a.c[k] > 0 && mlf_it(a, k).cat != MLF_ALONE) {
            // the item's own text, inside the concatenation's room
            uint8_t *cat0 = a.out + a.po[f] + pre, *cat1 = cat0 + (a.coff[L + 1] - a.coff[f]);
            uint8_t *d0 = cat0 + (a.coff[k] - a.coff[f]), *d1 = d0 + a.c[k];
            if (d1 > cat1) d1 = cat1;
            MlfSink s(d0 < cat1 ? d0 : cat1, d1);
            mlf_piece(s, a, k);
            if (s.over || s.p != d0 + a.c[k]) n_mis++;
        }
        if (dup) {
            uint8_t *d1 = a.out + a.po[k + 1], *d0 = d1 - dup;
            MlfSink s(d0, d1);
            if (!mlf_whole(s, a, k, a.tsec[k], a.tnsec[k]) || s.over || s.pos() != dup) n_mis++;
            a.rows_out[a.ridx[k] + (k == f ? 1 : 0)] = (uint64_t) (d0 - a.out);
        }
    }
    n_mis = lane_wave_sum(n_mis);
    if ((threadIdx.x & 63u) == 0 && n_mis) atomicAdd(&a.w->mismatch, n_mis);
}

// (a launch over no rows still runs one block: k_mlf_items writes the first item's columns)
static unsigned mlf_blocks(uint64_t n) { return lane_blocks<MLF_BLOCK>(n ? n : 1); }
void launch_mlf_class(const MlfArgs &a, hipStream_t st) { if (a.n) hipLaunchKernelGGL(k_mlf_class, dim3(mlf_blocks(a.n)), dim3(MLF_BLOCK), 0, st, a); }
void launch_mlf_items(const MlfArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_mlf_items, dim3(mlf_blocks(a.n)), dim3(MLF_BLOCK), 0, st, a); }
void launch_mlf_fix(const MlfArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_mlf_fix, dim3(mlf_blocks(a.N)), dim3(MLF_BLOCK), 0, st, a); }
void launch_mlf_plan(const MlfArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_mlf_plan, dim3(mlf_blocks(a.N)), dim3(MLF_BLOCK), 0, st, a); }
void launch_mlf_regidx(const MlfArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_mlf_regidx, dim3(mlf_blocks(2 * a.N)), dim3(MLF_BLOCK), 0, st, a); }
void launch_mlf_size(const MlfArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_mlf_size, dim3(mlf_blocks(a.N)), dim3(MLF_BLOCK), 0, st, a); }
void launch_mlf_emit(const MlfArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_mlf_emit, dim3(mlf_blocks(a.N)), dim3(MLF_BLOCK), 0, st, a); }
