// throttle_kernels.inc -- filter_throttle_size (plugins/filter_throttle_size/throttle_size.c:308-433 throttle_data_by_size, 169-192 the
// ticker; size_window.h:59-91): the windows live in HBM between calls, columns by window id, and the names in an L2mTable.
//   k_tsz_extract   a lane per record, both paths in LDS: name -> window id (inserting the name when new), load, record length.  It
//                   changes NO window: when the dictionary fills, the host grows it and the pass simply runs again.
//   k_tsz_keys      the sort's input: (window id, row) of the throttled rows, the others behind them
//   k_tsz_admit     the greedy admission over the rows of one name in record order, names side by side: <false> a lane per short
//                   segment (and the list of the long ones), <true> a wave per long segment.  The window's columns are written once,
//                   behind the segment's last row.
//   k_tsz_tick      a lane per window id: add_new_pane, then the stale test
// Every loop is bounded by a length (never by a sentinel); nothing recurses.  Included inside namespace flbgpu after kdev.inc,
// lane_rows.inc, ra_lds.inc and l2m_dev.inc.

// get_value_of_msgpack_object_map (:253-305) over `nparts` parts that start at part `p0` of the table: at each level the FIRST key
// that is STR or BIN with the part's length and bytes.  A level that is no map has no such key (DESIGN 8: the reference reads a
// value that is no map as one).  nullptr: not found.
DEV const uint8_t *tsz_path(const LDS_AS uint32_t *w, uint32_t p0, uint32_t nparts, const uint8_t *v, const uint8_t *end) {
    for (uint32_t i = 0; i < nparts; i++) {
        const uint32_t L = w[TSZ_HDR_WORDS + 2 * (p0 + i)];
        const LDS_AS uint32_t *bytes = w + (w[TSZ_HDR_WORDS + 2 * (p0 + i) + 1] >> 2);
        const Tok m = mp_tok(v, end);
        if (m.type != T_MAP) return nullptr;
        const uint8_t *p = m.next, *found = nullptr;
        for (uint32_t e = 0; e < m.len; e++) {
            const Tok k = mp_tok(p, end);
            const uint8_t *kend = mp_end_of(k, p, end, 0);
            if (!kend) return nullptr;
            if ((k.type == T_STR || k.type == T_BIN) && k.len == L && lds_eq(bytes, L, k.next)) { found = kend; break; }
            p = mp_skip(kend, end, 0);
            if (!p) return nullptr;
        }
        if (!found) return nullptr;
        v = found;
    }
    return v;
}

// get_msgpack_object_size (:220-246): the payload bytes of every STR and BIN inside the object, map keys included.  One counter of
// the elements still to come instead of a stack: the decoder has bounded the depth already.
DEV unsigned long long tsz_load(const uint8_t *p, const uint8_t *end) {
    unsigned long long sum = 0, remaining = 1;
    while (remaining > 0) {
        const Tok t = mp_tok(p, end);
        if (t.type == T_BAD) break;
        remaining--;
        p = t.next;
        if (t.type == T_STR || t.type == T_BIN) { sum += t.len; p += t.len; }
        else if (t.type == T_EXT) p += t.len;
        else if (t.type == T_ARRAY) remaining += t.len;
        else if (t.type == T_MAP) remaining += 2ull * t.len;
    }
    return sum;
}

struct TszName {
    const uint8_t *p;
    uint32_t len;
    template <class Sink> DEV void run(Sink &k) const { for (uint32_t j = 0; j < len; j++) k.put(ld8(p + j)); }
};

// A new name's room: its bytes in the arena and its id, each ONE atomic add that is never taken back.  l2m_reserve's compare-and-swap
// loops are right for a few thousand new series a call; a chunk of millions of new names has a hundred thousand lanes retrying on
// one word, and every success costs all the others a failed attempt.  An add cannot fail, so the cost is one atomic a name.  No
// room: the counter has run past its bound, which nobody reads as
// a count -- the host sees `overflow`, rebuilds the dictionary with fresh counters (throttle.cpp grow) and runs the pass again -- and
// ids and offsets below the bounds stay valid, because a counter that is never decremented hands out every value once.
DEV bool tsz_reserve(const L2mTable &t, uint32_t padded, uint32_t *sid_out, unsigned long long *off_out) {
    if (l2m_ld64(t.arena_used) + padded > t.arena_cap || l2m_ld32(t.n_series) >= t.max_series) return false;      // (full already: no add at all)
    const unsigned long long off = atomicAdd(t.arena_used, (unsigned long long) padded);
    if (off + padded > t.arena_cap) return false;
    const uint32_t sid = atomicAdd(t.n_series, 1u);
    if (sid >= t.max_series) return false;
    *sid_out = sid; *off_out = off;
    return true;
}

// window id of a name, inserting it when new: the dictionary protocol of sp_group_id over the same table type.  The hash keeps the
// bits of `mask` only (FLBGPU_TSZ_HASH_BITS): the byte comparison decides between names that share one.
DEV uint32_t tsz_name_id(const L2mTable &t, const TszName &nm, uint64_t mask) {
    L2mHashSink hs;
    nm.run(hs);
    uint64_t h = l2m_mix(hs.h) & mask;
    if (h < 2) h += 2;
    const uint32_t klen = hs.n;
    uint64_t pos = h & t.cap_mask;
    uint64_t probes = 0;
    while (probes <= t.cap_mask) {
        unsigned long long cur = l2m_ld64(&t.slot_hash[pos]);
        if (cur == h) {
            uint32_t sid = l2m_ld32(&t.slot_sid[pos]);
            if (l2m_ld32(&t.key_len[sid]) == klen) {
                L2mCmpSink cs(t.arena + l2m_ld64(&t.key_off[sid]), klen);
                nm.run(cs);
                if (cs.eq && cs.n == klen) return sid;
            }
            pos = (pos + 1) & t.cap_mask; probes++;
        }
        else if (cur == 0) {
            if (atomicCAS(&t.slot_hash[pos], 0ull, 1ull) == 0ull) {
                const uint32_t padded = (klen + 7) & ~7u;
                uint32_t sid = 0;
                unsigned long long off = 0;
                if (!tsz_reserve(t, padded, &sid, &off)) {
                    atomicExch(t.overflow, 1u);
                    l2m_st64(&t.slot_hash[pos], 0ull);
                    return TSZ_NONE;
                }
                L2mStoreSink ss(t.arena + off);
                nm.run(ss);
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
    return TSZ_NONE;
}

// the reference's comparison (:377-378, :414-416) in binary64 exactly as it is written there: convert, divide, subtract, compare
// (this unit is compiled without contraction)
DEV bool tsz_over(unsigned long long sum, uint32_t window, double rate) {
    const double current_rate = (double) sum / (double) window;
    return current_rate - rate > 0.001;
}

__global__ void __launch_bounds__(TSZ_BLOCK) k_tsz_extract(TszArgs a) {
    LDS_AS uint32_t *w = lane_stage_table<TSZ_BLOCK>(a.table, a.table_bytes);
    __syncthreads();
    const uint32_t nname = w[0], nlog = w[1];
    unsigned long long n_rec = 0, n_exempt = 0, n_big = 0, n_thr = 0, n_alone = 0;
    lane_wave_rows<TSZ_BLOCK>(a.n, [&](uint64_t r, bool live) {
        uint32_t wid = TSZ_UNSEEN, len = 0;
        unsigned long long load = 0;
        bool rec_seen = false;
        if (live) {
            const uint8_t *rec = a.data + a.row_off[r], *end = a.data + a.row_off[r + 1];
            if (rec != end) {                                               // (an empty row: a record an earlier filter dropped)
                const Event ev = decode_event(rec, end, false);
                if ((ev.flags & RF_BAD) || ev.body_end != end) atomicMin(&a.firsts[0], (unsigned long long) r);
                else if (!(ev.flags & RF_SKIP)) {                           // (group markers: the decoder's loop steps over them)
                    rec_seen = true;
                    const uint64_t raw = (uint64_t) (end - rec);
                    if (raw > 0xFFFFFFFFull) n_big++;
                    len = (uint32_t) raw;
                    wid = TSZ_EXEMPT;
                    TszName nm{nullptr, 0};
                    bool named = nname == 0 && a.load;
                    if (nname) {
                        const uint8_t *v = tsz_path(w, 0, nname, ev.body, end);
                        if (v) {
                            const Tok t = mp_tok(v, end);
                            if (t.type == T_STR || t.type == T_BIN) { nm.p = t.next; nm.len = t.len; named = true; }
                        }
                    }
                    if (named) {
                        const uint8_t *lv = nlog ? tsz_path(w, nname, nlog, ev.body, end) : ev.body;
                        if (lv) {
                            load = tsz_load(lv, end);
                            if (nname == 0) wid = 0;                                        // (`*` is name 0 from create on)
                            else if (nm.len == 0) {
                                // an empty name: flb_hash_table_get and flb_hash_table_add both refuse a key of no bytes, so the
                                // record never finds a window and never leaves one: it is judged alone, every time (:370-383)
                                if (tsz_over(load, a.window, a.rate)) { wid = TSZ_UNSEEN; len = 0; n_alone++; }
                            }
                            else wid = tsz_name_id(a.t, nm, a.hash_mask);
                        }
                    }
                }
            }
            if (a.load) { a.wid[r] = wid; a.load[r] = load; }
            else a.wid[r] = rec_seen ? 1u : 0u;                             // filter_throttle: the rows are only told apart
            a.len[r] = len;
        }
        lane_count(n_rec, rec_seen);
        lane_count(n_exempt, rec_seen && wid == TSZ_EXEMPT);
        lane_count(n_thr, rec_seen && wid < TSZ_NONE);
    });
    lane_flush(&a.counts[0], n_rec); lane_flush(&a.counts[1], n_exempt); lane_flush(&a.counts[2], n_big); lane_flush(&a.counts[3], n_thr);
    n_alone = lane_wave_sum(n_alone);
    if ((threadIdx.x & 63u) == 0) lane_flush(&a.counts[4], n_alone);
}

void launch_tsz_extract(const TszArgs &a, hipStream_t st) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_tsz_extract, dim3(lane_blocks<TSZ_BLOCK>(a.n)), dim3(TSZ_BLOCK), a.table_bytes, st, a);
}

// ---- order
__global__ void __launch_bounds__(256) k_tsz_keys(const uint32_t *wid, uint64_t n, uint32_t nids, uint32_t *keys, uint32_t *rows) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t k = wid[i];
        keys[i] = k < nids ? k : nids;
        rows[i] = (uint32_t) i;
    }
}

// ---- admission
// what a segment leaves in its window: `total` as the last kept record left it, the kept loads' sum for the newest pane
struct TszSeg {
    bool exists, kept_any, nonzero;
    unsigned long long total, added;
};

DEV TszSeg tsz_seg_open(const TszWindows &w, uint32_t id) {
    TszSeg s;
    s.exists = w.exists[id] != 0;
    s.kept_any = false; s.nonzero = false;
    s.total = s.exists ? w.total[id] : 0;       // no window yet: the record is judged alone (:377) until one is kept
    s.added = 0;
    return s;
}

// size_window_create (size_window.c:42-91) where the segment's first kept record met no window, then add_load (size_window.h:83-91)
// for all of the segment's kept records at once: they all went into the same newest pane.  Returns 1 when it created the window.
DEV uint32_t tsz_seg_close(const TszWindows &w, uint32_t id, const TszSeg &s, long long now) {
    if (!s.kept_any) return 0;
    uint32_t created = 0;
    if (!s.exists) {
        for (uint32_t p = 0; p < w.window; p++) { w.pane_ts[(uint64_t) id * w.window + p] = now; w.pane_size[(uint64_t) id * w.window + p] = 0; }
        w.head[id] = (int32_t) w.window - 1;
        w.tail[id] = 0;
        w.timestamp[id] = now;
        w.exists[id] = 1;
        created = 1;
    }
    const uint64_t hp = (uint64_t) id * w.window + (uint32_t) w.head[id];
    w.pane_size[hp] += s.added;
    w.total[id] = s.total;
    if (s.nonzero) w.timestamp[id] = w.pane_ts[hp];
    return created;
}

DEV unsigned long long tsz_wave_scan(unsigned long long v, uint32_t lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o, 64);
        if (lane >= (uint32_t) o) v += t;
    }
    return v;
}

// WAVE false: a lane per sorted position; the lane that stands on a segment's first row walks the segment when it is shorter than
// wave_min and lists it otherwise.  WAVE true: a wave (= a block) per listed segment, 64 consecutive rows a trip.  Every lane of the
// wave runs every ballot and every shuffle of a trip: what a trip does next depends on wave-uniform values only (ballots, lane 0's
// broadcast), and a lane past the segment's end takes part with a load of 0 and is never looked at.
template <bool WAVE>
__global__ void __launch_bounds__(WAVE ? 64 : 256) k_tsz_admit(TszAdmitArgs a) {
    unsigned long long n_drop = 0, n_new = 0;
    if (!WAVE) {
        for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += (uint64_t) gridDim.x * blockDim.x) {
            const uint32_t k = a.keys[i];
            if (i && a.keys[i - 1] == k) continue;
            uint64_t e = i + 1;
            while (e < a.m && e - i < a.wave_min && a.keys[e] == k) e++;
            if (e - i >= a.wave_min) { a.heavy[atomicAdd(a.nheavy, 1u)] = (uint32_t) i; continue; }
            TszSeg s = tsz_seg_open(a.w, k);
            for (uint64_t j = i; j < e; j++) {
                const uint32_t row = a.rows[j];
                const unsigned long long L = a.load[row];
                if (tsz_over(s.total + L, a.w.window, a.rate)) { a.len[row] = 0; n_drop++; }
                else { s.total += L; s.added += L; s.kept_any = true; s.nonzero = s.nonzero || L != 0; }
            }
            n_new += tsz_seg_close(a.w, k, s, a.now);
        }
    }
    else {
        const uint32_t lane = threadIdx.x;
        const uint32_t nheavy = *a.nheavy;
        for (uint32_t h = blockIdx.x; h < nheavy; h += gridDim.x) {
            const uint64_t b = a.heavy[h];
            const uint32_t k = a.keys[b];
            TszSeg s = tsz_seg_open(a.w, k);                             // (every lane reads the same words)
            for (uint64_t i0 = b; ; i0 += 64) {
                const uint64_t i = i0 + lane;
                const bool live = i < a.m && a.keys[i] == k;
                const unsigned long long lb = __ballot(live);
                // (the segment is one run of the sorted keys: the live lanes are the first `nlive` of the trip)
                const uint32_t nlive = (uint32_t) __popcll(lb);
                if (nlive == 0) break;
                const uint32_t row = live ? a.rows[i] : 0u;
                const unsigned long long L = live ? a.load[row] : 0ull;
                const unsigned long long P = tsz_wave_scan(L, lane);     // inclusive prefix of the trip's loads
                bool keep = false;
                uint32_t pos = 0;                                        // the first row of the trip that is not decided yet
                while (pos < nlive) {
                    // rows pos .. : the prefix from pos on top of the total.  The comparison is monotone in the sum, so the first
                    // lane that is over is the first row that does not fit, and every row in front of it is kept
                    const unsigned long long base = pos ? __shfl(P, (int) pos - 1, 64) : 0ull;
                    const bool in = live && lane >= pos;
                    const unsigned long long over = __ballot(in && tsz_over(s.total + (P - base), a.w.window, a.rate));
                    const uint32_t f = over ? (uint32_t) __ffsll((long long) over) - 1 : nlive;
                    if (in && lane < f) keep = true;
                    if (f > pos) {
                        const unsigned long long upto = __shfl(P, (int) f - 1, 64) - base;
                        const unsigned long long nz = __ballot(in && lane < f && L != 0);
                        s.total += upto; s.added += upto; s.kept_any = true; s.nonzero = s.nonzero || nz != 0;
                    }
                    if (f >= nlive) break;
                    // row f is dropped.  With the capacity that is left, the next kept row is the first one behind it whose own
                    // load still fits; the stretch in front of that row is dropped in one step, and so is a stretch without one
                    const unsigned long long fits = __ballot(live && lane > f && !tsz_over(s.total + L, a.w.window, a.rate));
                    pos = fits ? (uint32_t) __ffsll((long long) fits) - 1 : nlive;
                }
                if (live && !keep) a.len[row] = 0;
                const unsigned long long dropped = __ballot(live && !keep);
                if (lane == 0) n_drop += __popcll(dropped);
                if (nlive < 64) break;
            }
            if (lane == 0) n_new += tsz_seg_close(a.w, k, s, a.now);
        }
    }
    // (the row loops are over: the whole wave is here again)
    n_drop = lane_wave_sum(n_drop); n_new = lane_wave_sum(n_new);
    if ((threadIdx.x & 63u) == 0) { lane_flush(&a.counts[0], n_drop); lane_flush(&a.counts[1], n_new); }
}

namespace {
struct TszLayout { uint64_t n; size_t keys_in, rows_in, keys_out, rows_out, heavy, nheavy, sort_tmp, total, sort_bytes; };
// The work buffer of one call over n rows.  The layout -- and rocPRIM's answer about its temporary storage -- is kept for the last n
// asked about: a call asks twice.  The storage is asked for a sort over all 32 bits while the sort itself runs over as many bits as
// the dictionary needs: fewer bits never need more storage, so the buffer is at least as large as the sort wants.
TszLayout tsz_layout(uint64_t n) {
    static thread_local TszLayout last = {~0ull, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (last.n == n) return last;
    TszLayout l;
    l.n = n;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t) 255; return o; };
    l.keys_in = take(n * 4); l.rows_in = take(n * 4); l.keys_out = take(n * 4); l.rows_out = take(n * 4); l.heavy = take(n * 4); l.nheavy = take(16);
    size_t tmp = 0;
    (void) rocprim::radix_sort_pairs(nullptr, tmp, (const uint32_t *) nullptr, (uint32_t *) nullptr, (const uint32_t *) nullptr, (uint32_t *) nullptr, (size_t) n, 0u, 32u);
    l.sort_bytes = tmp;
    l.sort_tmp = take(tmp);
    l.total = at;
    last = l;
    return l;
}
}  // namespace

size_t tsz_order_bytes(uint64_t n) { return tsz_layout(n).total; }

// the rows in (window id, row) order: the throttled rows first (a.m of them: k_tsz_extract counted them), the others behind them.
// Fills in a.keys, a.rows and the list of long segments.  false: the sort failed
bool launch_tsz_order(TszAdmitArgs &a, const uint32_t *wid, uint64_t n, uint32_t nids, void *work, size_t work_bytes, hipStream_t st) {
    if (n == 0 || a.m == 0) return true;
    const TszLayout l = tsz_layout(n);
    if (work_bytes < l.total || a.m > n) return false;
    uint8_t *w = (uint8_t *) work;
    uint32_t *keys_in = (uint32_t *) (w + l.keys_in), *rows_in = (uint32_t *) (w + l.rows_in);
    uint32_t *keys_out = (uint32_t *) (w + l.keys_out), *rows_out = (uint32_t *) (w + l.rows_out);
    const unsigned blocks = (unsigned) ((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_tsz_keys, dim3(blocks), dim3(256), 0, st, wid, n, nids, keys_in, rows_in);
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) <= (unsigned long long) nids) bits++;            // keys 0 .. nids
    size_t tmp = l.sort_bytes;
    if (rocprim::radix_sort_pairs(w + l.sort_tmp, tmp, (const uint32_t *) keys_in, keys_out, (const uint32_t *) rows_in, rows_out, (size_t) n, 0u, bits, st) != hipSuccess)
        return false;
    a.keys = keys_out; a.rows = rows_out;
    a.heavy = (uint32_t *) (w + l.heavy); a.nheavy = (unsigned int *) (w + l.nheavy);
    return hipMemsetAsync(a.nheavy, 0, 16, st) == hipSuccess && hipGetLastError() == hipSuccess;
}

// behind launch_tsz_order: wave false -- the short segments, a lane each, and the list of the long ones; wave true -- the listed ones
void launch_tsz_admit(const TszAdmitArgs &a, bool wave, hipStream_t st) {
    if (a.m == 0) return;
    if (!wave) {
        const unsigned ablocks = (unsigned) ((a.m + 255) / 256 < 4096 ? (a.m + 255) / 256 : 4096);
        hipLaunchKernelGGL(k_tsz_admit<false>, dim3(ablocks), dim3(256), 0, st, a);
        return;
    }
    const uint64_t most = a.m / (a.wave_min ? a.wave_min : 1) + 1;                      // no more long segments than this
    hipLaunchKernelGGL(k_tsz_admit<true>, dim3((unsigned) (most < 1024 ? most : 1024)), dim3(64), 0, st, a);
}

// ---- the ticker's trip (:169-192): add_new_pane for every window (size_window.h:59-77), then the stale ones go (:107-149)
__global__ void __launch_bounds__(256) k_tsz_tick(TszTickArgs a) {
    unsigned long long n_live = 0, n_del = 0;
    for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < a.nids; id += gridDim.x * blockDim.x) {
        if (!a.w.exists[id]) continue;
        const uint64_t p0 = (uint64_t) id * a.w.window;
        int32_t head = a.w.head[id], tail = a.w.tail[id];
        const unsigned long long tail_size = a.w.pane_size[p0 + (uint32_t) tail];
        if ((int32_t) a.w.window - 1 == head) head = -1;
        head += 1;
        a.w.pane_ts[p0 + (uint32_t) head] = a.ts;
        a.w.pane_size[p0 + (uint32_t) head] = 0;
        a.w.total[id] -= tail_size;
        if ((int32_t) a.w.window - 1 == tail) tail = -1;
        tail += 1;
        a.w.head[id] = head; a.w.tail[id] = tail;
        if (a.threshold > a.w.timestamp[id]) { a.w.exists[id] = 0; n_del++; }
        else n_live++;
    }
    n_live = lane_wave_sum(n_live); n_del = lane_wave_sum(n_del);
    if ((threadIdx.x & 63u) == 0) { lane_flush(&a.counts[0], n_live); lane_flush(&a.counts[1], n_del); }
}

// filter_throttle keeps a call's first K records: idx = the records in front of each row (a scan over k_tsz_extract's flags)
__global__ void __launch_bounds__(256) k_thr_first(uint32_t *len, const uint64_t *idx, uint64_t K, uint64_t n) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        if (idx[i] >= K) len[i] = 0;
}

void launch_thr_first(uint32_t *len, const uint64_t *idx, uint64_t K, uint64_t n, hipStream_t st) {
    if (n == 0) return;
    const unsigned blocks = (unsigned) ((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_thr_first, dim3(blocks), dim3(256), 0, st, len, idx, K, n);
}

void launch_tsz_tick(const TszTickArgs &a, hipStream_t st) {
    if (a.nids == 0) return;
    const unsigned blocks = (a.nids + 255) / 256 < 4096 ? (a.nids + 255) / 256 : 4096;
    hipLaunchKernelGGL(k_tsz_tick, dim3(blocks), dim3(256), 0, st, a);
}
