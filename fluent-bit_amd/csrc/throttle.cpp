// throttle.cpp -- filter_throttle_size (plugins/filter_throttle_size/throttle_size.c) and filter_throttle (plugins/filter_throttle/
// throttle.c, window.c): the configuration as configure / the config map read it, the names' dictionary and the windows' columns in
// HBM with their growth, one cb_filter call on a device chunk, one trip of the ticker.  The per-record work is throttle_kernels.inc.
#include <cctype>
#include <climits>
#include <mutex>
#include "filter_host.hpp"
#include "throttle.hpp"

using namespace flbgpu;

namespace {

// ---- what the reference's helpers accept, restated (the recording pins them)

// flb_utils_size_to_bytes (src/flb_utils.c:527-608)
int64_t size_to_bytes(const char *size) {
    if (!strcasecmp(size, "false")) return 0;
    const int len = (int) strlen(size);
    const double val = atof(size);
    if (len == 0) return -1;
    int plen = 0;
    for (int i = len - 1; i > 0; i--) {
        if (isdigit((unsigned char) size[i])) break;
        plen++;
    }
    // (a double the int64 cannot hold is undefined in the reference: it reads as "not positive" here)
    auto to_i64 = [](double v) { return v >= 9223372036854775808.0 || v <= -9223372036854775808.0 || v != v ? (int64_t) -1 : (int64_t) v; };
    if (plen == 0) return to_i64(val);
    if (plen > 2) return -1;
    char tmp[3] = {0, 0, 0};
    for (int i = 0; i < plen; i++) tmp[i] = (char) toupper((unsigned char) size[(len - plen) + i]);
    if (plen == 2 && tmp[1] != 'B') return -1;
    if (tmp[0] == 'K') return (val >= 9223372036854775.0 || val <= -9223372036854774.0) ? -1 : to_i64(val * 1000);
    if (tmp[0] == 'M') return (val >= 9223372036854 || val <= -9223372036853) ? -1 : to_i64(val * 1000000);
    if (tmp[0] == 'G') return (val >= 9223372036 || val <= -9223372035) ? -1 : to_i64(val * 1000000000);
    return -1;
}

// flb_utils_split(line, sep, max_split) (src/flb_utils.c:321-457, no quotes): leading separators of a token are stepped over, a
// token ends at the next separator, and behind max_split tokens the rest of the line is one more entry as it stands
void utils_split(const std::string &line, char sep, int max_split, std::vector<std::string> &out) {
    out.clear();
    const int len = (int) line.size();
    int i = 0, count = 0;
    while (i < len) {
        int t = i;
        while (t < len && line[t] == sep) t++;
        int e = t;
        while (e < len && line[e] != sep) e++;
        out.push_back(line.substr(t, e - t));
        count++;
        i = e + 1;
        if (count >= max_split && max_split > 0 && i < len) { out.push_back(line.substr(i)); break; }
    }
}

// flb_utils_bool (src/flb_utils.c:757-): 1, 0 or -1
int utils_bool(const char *v) {
    if (!strcasecmp(v, "true") || !strcasecmp(v, "on") || !strcasecmp(v, "yes")) return 1;
    if (!strcasecmp(v, "false") || !strcasecmp(v, "off") || !strcasecmp(v, "no")) return 0;
    return -1;
}

bool apply_suffix(double *x, char c) {
    int m;
    switch (c) {
    case 0: case 's': m = 1; break;
    case 'm': m = 60; break;
    case 'h': m = 3600; break;
    case 'd': m = 86400; break;
    default: return false;
    }
    *x *= m;
    return true;
}

// the first value of a property, names without case (flb_filter_get_property)
const char *prop(int nprops, const char *const *names, const char *const *values, const char *name) {
    for (int i = 0; i < nprops; i++) if (names[i] && !strcasecmp(names[i], name)) return values[i] ? values[i] : "";
    return nullptr;
}

struct TszConfig {
    double rate = 1048576.0;
    uint32_t window = 5;
    int interval = 1, duration = 60;
    std::vector<std::string> name_parts, log_parts;
};

// throttle_size.c parse_duration (:478-499); false: a value an int cannot hold
bool tsz_duration(const char *text, int def, int &out, std::string &why) {
    char *p;
    double s = strtod(text, &p);
    if (0 >= s || (*p && *(p + 1)) || !apply_suffix(&s, *p)) { out = def; return true; }
    if (!(s < 2147483648.0)) { why = std::string("'") + text + "': more seconds than an int holds"; return false; }
    out = (int) s;
    return true;
}

// configure (:501-597) and the raise of cb_throttle_size_init (:621-623)
bool tsz_parse(int nprops, const char *const *names, const char *const *values, TszConfig &c, std::string &why) {
    if (const char *s = prop(nprops, names, values, "rate")) {
        const int64_t bytes = size_to_bytes(s);
        if (bytes > 0) c.rate = (double) bytes;
    }
    if (const char *s = prop(nprops, names, values, "window")) {
        char *endp;
        const double val = (double) strtoul(s, &endp, 10);
        if (val > 1) {
            if (val > 65536) { why = std::string("window '") + s + "': more than 65536 panes"; return false; }
            c.window = (uint32_t) val;
        }
    }
    if (const char *s = prop(nprops, names, values, "interval")) if (!tsz_duration(s, 1, c.interval, why)) return false;
    if (const char *s = prop(nprops, names, values, "log_field")) utils_split(s, '|', 20, c.log_parts);
    if (const char *s = prop(nprops, names, values, "name_field")) utils_split(s, '|', 20, c.name_parts);
    if (const char *s = prop(nprops, names, values, "window_time_duration")) if (!tsz_duration(s, 60, c.duration, why)) return false;
    const int64_t least = (int64_t) c.interval * (int64_t) c.window;
    if (least > INT_MAX) { why = "interval * window: more seconds than an int holds"; return false; }
    if ((int64_t) c.duration < least) c.duration = (int) least;
    return true;
}

std::string fmt_g(double v) { char b[64]; snprintf(b, sizeof(b), "%.17g", v); return b; }

std::string describe_path(const std::vector<std::string> &parts) {
    if (parts.empty()) return "-";
    std::string d;
    for (size_t i = 0; i < parts.size(); i++) d += (i ? "|" : "") + hexs(parts[i]);
    return d;
}

std::string tsz_describe(const TszConfig &c) {
    return "rate=" + fmt_g(c.rate) + ";window=" + std::to_string(c.window) + ";interval=" + std::to_string(c.interval) + ";duration=" +
           std::to_string(c.duration) + ";name=" + describe_path(c.name_parts) + ";log=" + describe_path(c.log_parts);
}

// the LDS table of throttle.hpp
void tsz_table(const TszConfig &c, std::vector<uint32_t> &t) {
    const size_t np = c.name_parts.size() + c.log_parts.size();
    t.assign(TSZ_HDR_WORDS + 2 * np, 0);
    t[0] = (uint32_t) c.name_parts.size(); t[1] = (uint32_t) c.log_parts.size();
    for (size_t i = 0; i < np; i++) {
        const std::string &s = i < c.name_parts.size() ? c.name_parts[i] : c.log_parts[i - c.name_parts.size()];
        t[TSZ_HDR_WORDS + 2 * i] = (uint32_t) s.size();
        t[TSZ_HDR_WORDS + 2 * i + 1] = (uint32_t) (t.size() * 4);
        for (size_t j = 0; j < s.size(); j += 4) {
            uint32_t w = 0;
            for (size_t b = 0; b < 4 && j + b < s.size(); b++) w |= (uint32_t) (unsigned char) s[j + b] << (8 * b);
            t.push_back(w);
        }
    }
}

bool tsz_checked(int nprops, const char *const *names, const char *const *values, TszConfig &c, std::vector<uint32_t> &table) {
    if (!parse_front("throttle_size", nprops, names, values, [&](std::string &why) { return tsz_parse(nprops, names, values, c, why); })) return false;
    tsz_table(c, table);
    if (table.size() * 4 > TC_MAX_TABLE_BYTES) { set_err("filter_throttle_size: path table larger than %u bytes", TC_MAX_TABLE_BYTES); return false; }
    return true;
}

uint64_t env_u64(const char *name, uint64_t def, uint64_t lo, uint64_t hi) {
    const char *e = getenv(name);
    char *end = nullptr;
    const unsigned long long v = e ? strtoull(e, &end, 10) : 0;
    return (e && end != e && *end == 0 && v >= lo && v <= hi) ? (uint64_t) v : def;
}

// the hash of a name as k_tsz_extract forms it (l2m_dev.inc: FNV-1a, l2m_mix)
uint64_t name_hash(const uint8_t *p, size_t n, uint64_t mask) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    h ^= h >> 32; h *= 0x9E3779B97F4A7C15ull; h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    if (h < 2) h += 2;
    h &= mask;
    return h < 2 ? h + 2 : h;
}

bool fresh(DevBuf &b, size_t bytes) {
    b.release();
    if (!b.ensure(bytes + 16)) return false;
    HIPOK(hipMemset(b.p, 0, b.cap));
    return true;
}
template <class T> bool put(DevBuf &b, const std::vector<T> &v) {
    if (!v.empty()) HIPOK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return true;
}
template <class T> bool get(std::vector<T> &v, const DevBuf &b, size_t n) {
    v.resize(n);
    if (n) HIPOK(hipMemcpy(v.data(), b.p, n * sizeof(T), hipMemcpyDeviceToHost));
    return true;
}

// the windows of `ids` names as the host holds them while it rebuilds or shows them
struct HostWindows {
    std::vector<uint32_t> exists;
    std::vector<unsigned long long> total, pane_size, key_off;
    std::vector<long long> timestamp, pane_ts;
    std::vector<int32_t> head, tail;
    std::vector<uint32_t> key_len;
    std::vector<uint8_t> arena;
};

struct TszState : FilterState {
    struct Words { unsigned long long firsts[1], counts[5], adm[2]; };
    std::mutex mu;
    TszConfig cfg;
    uint32_t table_bytes = 0;
    uint64_t hash_mask = ~0ull;
    uint32_t wave_min = TSZ_WAVE_MIN;
    // the names: an L2mTable (dev.hpp) -- slots, arena, per-id descriptors, counters
    uint64_t cap = 0, arena_cap = 0;
    uint32_t max_ids = 0, nids = 0;
    ScopedDevBuf d_slot_hash, d_slot_sid, d_arena, d_key_off, d_key_len, d_id_hash, d_ctr;
    // the windows, columns by id (max_ids of each)
    ScopedDevBuf d_exists, d_total, d_ts, d_head, d_tail, d_pane_ts, d_pane_size;
    ScopedDevBuf d_table, d_wid, d_load, d_work;
    CallWords<Words> words;
    int64_t now = 0;
    bool started = false;
    // HIP's current device is the calling thread's: every entry a caller's timer thread may use selects the filter's own first
    int device = 0;
    bool on_device() const { HIPOK(hipSetDevice(device)); return true; }
    uint64_t n_in = 0, n_kept = 0, n_dropped = 0, n_exempt = 0, live = 0, created = 0, deleted = 0, grows = 0;
    // the view of flbgpu_throttle_size_windows
    std::string v_names;
    std::vector<uint64_t> v_name_off, v_total, v_pane_size;
    std::vector<int64_t> v_ts, v_pane_ts;
    std::vector<int32_t> v_head;

    L2mTable table_of() const {
        L2mTable t;
        L2mCtr *c = d_ctr.as<L2mCtr>();
        t.slot_hash = d_slot_hash.as<unsigned long long>(); t.slot_sid = d_slot_sid.as<uint32_t>();
        t.cap_mask = cap - 1; t.max_series = max_ids; t.n_series = &c->n_series;
        t.arena = d_arena.as<uint8_t>(); t.arena_used = &c->arena_used; t.arena_cap = arena_cap;
        t.key_off = d_key_off.as<unsigned long long>(); t.key_len = d_key_len.as<uint32_t>(); t.series_hash = d_id_hash.as<unsigned long long>();
        t.overflow = &c->overflow;
        return t;
    }
    TszWindows windows_of() const {
        TszWindows w;
        w.exists = d_exists.as<uint32_t>(); w.total = d_total.as<unsigned long long>(); w.timestamp = d_ts.as<long long>();
        w.head = d_head.as<int32_t>(); w.tail = d_tail.as<int32_t>(); w.pane_ts = d_pane_ts.as<long long>();
        w.pane_size = d_pane_size.as<unsigned long long>(); w.window = cfg.window;
        return w;
    }
    // (a pass that ran out of room leaves its counters past their bounds: tsz_reserve never takes an add back)
    void clip(L2mCtr &c) const { if (c.n_series > max_ids) c.n_series = max_ids; if (c.arena_used > arena_cap) c.arena_used = arena_cap; }
    bool download(HostWindows &h, uint32_t ids, uint64_t arena_used);
    bool rebuild(const HostWindows &h, uint32_t ids, uint64_t new_cap, uint64_t new_arena);
    bool grow();
    bool stamp_star(int64_t ts);
    bool redate_star(int64_t ts);
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
    bool tick(flbgpu_filter *f, int64_t seconds);
    bool view(flbgpu_tsz_windows *out);
};

bool TszState::download(HostWindows &h, uint32_t ids, uint64_t arena_used) {
    const size_t W = cfg.window;
    return get(h.exists, d_exists, ids) && get(h.total, d_total, ids) && get(h.timestamp, d_ts, ids) && get(h.head, d_head, ids) &&
           get(h.tail, d_tail, ids) && get(h.pane_ts, d_pane_ts, ids * W) && get(h.pane_size, d_pane_size, ids * W) &&
           get(h.key_off, d_key_off, ids) && get(h.key_len, d_key_len, ids) && get(h.arena, d_arena, (size_t) arena_used);
}

// The dictionary and the columns anew from the first `ids` names of h, of which only those whose window exists are entered: a dead
// name loses its id, and a later record of that name meets "no window" either way.  Ids are handed out again in the old order.
bool TszState::rebuild(const HostWindows &h, uint32_t ids, uint64_t new_cap, uint64_t new_arena) {
    const size_t W = cfg.window;
    const uint32_t new_max = (uint32_t) (new_cap / 2);
    std::vector<unsigned long long> slot_hash(new_cap, 0), key_off, id_hash, total, pane_size;
    std::vector<uint32_t> slot_sid(new_cap, 0), key_len, exists;
    std::vector<long long> ts, pane_ts;
    std::vector<int32_t> head, tail;
    std::vector<uint8_t> arena;
    for (uint32_t i = 0; i < ids; i++) {
        if (!h.exists[i]) continue;
        const uint32_t id = (uint32_t) key_off.size();
        const uint8_t *name = h.arena.data() + h.key_off[i];
        const uint64_t hv = name_hash(name, h.key_len[i], hash_mask);
        uint64_t pos = hv & (new_cap - 1);
        while (slot_hash[pos]) pos = (pos + 1) & (new_cap - 1);
        slot_hash[pos] = hv; slot_sid[pos] = id;
        key_off.push_back(arena.size()); key_len.push_back(h.key_len[i]); id_hash.push_back(hv);
        arena.insert(arena.end(), name, name + h.key_len[i]);
        arena.resize((arena.size() + 7) & ~(size_t) 7, 0);
        exists.push_back(1); total.push_back(h.total[i]); ts.push_back(h.timestamp[i]); head.push_back(h.head[i]); tail.push_back(h.tail[i]);
        pane_ts.insert(pane_ts.end(), h.pane_ts.begin() + i * W, h.pane_ts.begin() + (i + 1) * W);
        pane_size.insert(pane_size.end(), h.pane_size.begin() + i * W, h.pane_size.begin() + (i + 1) * W);
    }
    if (key_off.size() > new_max || arena.size() > new_arena) { set_err("filter_throttle_size: the rebuilt dictionary does not fit"); return false; }
    cap = new_cap; max_ids = new_max; arena_cap = new_arena; nids = (uint32_t) key_off.size();
    L2mCtr c;
    c.arena_used = arena.size(); c.n_series = nids; c.overflow = 0;
    if (!fresh(d_slot_hash, cap * 8) || !fresh(d_slot_sid, cap * 4) || !fresh(d_arena, arena_cap + 8) || !fresh(d_key_off, (size_t) max_ids * 8) ||
        !fresh(d_key_len, (size_t) max_ids * 4) || !fresh(d_id_hash, (size_t) max_ids * 8) || !fresh(d_ctr, sizeof(L2mCtr)) ||
        !fresh(d_exists, (size_t) max_ids * 4) || !fresh(d_total, (size_t) max_ids * 8) || !fresh(d_ts, (size_t) max_ids * 8) ||
        !fresh(d_head, (size_t) max_ids * 4) || !fresh(d_tail, (size_t) max_ids * 4) || !fresh(d_pane_ts, (size_t) max_ids * W * 8) ||
        !fresh(d_pane_size, (size_t) max_ids * W * 8))
        return false;
    HIPOK(hipMemcpy(d_ctr.p, &c, sizeof(c), hipMemcpyHostToDevice));
    return put(d_slot_hash, slot_hash) && put(d_slot_sid, slot_sid) && put(d_arena, arena) && put(d_key_off, key_off) && put(d_key_len, key_len) &&
           put(d_id_hash, id_hash) && put(d_exists, exists) && put(d_total, total) && put(d_ts, ts) && put(d_head, head) && put(d_tail, tail) &&
           put(d_pane_ts, pane_ts) && put(d_pane_size, pane_size);
}

// doubles whatever ran out (ids and / or arena, as l2m_table_grow does); the names without a window are not carried over
bool TszState::grow() {
    L2mCtr c;
    HIPOK(hipMemcpy(&c, d_ctr.p, sizeof(c), hipMemcpyDeviceToHost));
    clip(c);
    bool ids_full = (uint64_t) c.n_series * 2 >= max_ids, arena_full = c.arena_used * 2 >= arena_cap;
    if (!ids_full && !arena_full) ids_full = arena_full = true;       // a long probe run or one very long name
    HostWindows h;
    if (!download(h, c.n_series, c.arena_used)) return false;
    const uint64_t new_cap = ids_full ? cap * 2 : cap;
    if ((new_cap / 2) * (uint64_t) cfg.window * 16 > ((uint64_t) 16 << 30)) {
        set_err("filter_throttle_size: %u names with a window of %u panes each would take more than 16 GiB of panes", (unsigned) (new_cap / 2), cfg.window);
        return false;
    }
    grows++;
    return rebuild(h, c.n_series, new_cap, arena_full ? arena_cap * 2 : arena_cap);
}

// size_window_create for the `*` window (:630-641): id 0, every pane { ts, 0 }
bool TszState::stamp_star(int64_t ts) {
    HostWindows h;
    const size_t W = cfg.window;
    h.exists = {1}; h.total = {0}; h.timestamp = {ts}; h.head = {(int32_t) W - 1}; h.tail = {0};
    h.pane_ts.assign(W, ts); h.pane_size.assign(W, 0);
    h.key_off = {0}; h.key_len = {1}; h.arena = {'*', 0, 0, 0, 0, 0, 0, 0};
    return rebuild(h, 1, cap, arena_cap);
}

// the `*` window of create dated anew before anything ran: only the timestamps of id 0 differ, so only they are uploaded
bool TszState::redate_star(int64_t ts) {
    const std::vector<long long> stamp(1, ts), panes(cfg.window, ts);
    return put(d_ts, stamp) && put(d_pane_ts, panes);
}

int64_t clock_now() { return (int64_t) time(nullptr); }

// cb_throttle_size_filter (:659-736) on a device chunk.  Launch order: extract (again while the dictionary had to grow) -> sort by
// window id -> admit -> [a record was dropped: scan(kept bytes) -> copy].  The decoder's loop ends at the first record it refuses:
// the rows in front of it are the call, and what the loop kept of them goes out all the same (`garbage` changes nothing here).
bool TszState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool) {
    std::lock_guard<std::mutex> lock(mu);
    uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (!on_device()) return false;
    started = true;
    if (n == 0) return true;
    if (n > 0xFFFFFFF0ull) { set_err("filter_throttle_size: more than 2^32 rows in one call"); return false; }
    if (!words.ensure() || !ensure_row_columns(f, n) || !d_wid.ensure(n * 4) || !d_load.ensure(n * 8) || !d_work.ensure(tsz_order_bytes(n))) return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    uint64_t &total = words.total();
    TszArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = table_bytes; a.hash_mask = hash_mask; a.rate = cfg.rate; a.window = cfg.window;
    a.wid = d_wid.as<uint32_t>(); a.load = d_load.as<unsigned long long>(); a.len = f->d_len.as<uint32_t>();
    a.firsts = dw->firsts; a.counts = dw->counts;
    L2mCtr hc;
    for (int attempt = 0; ; attempt++) {
        if (attempt > 60) { set_err("filter_throttle_size: the name dictionary keeps overflowing"); return false; }
        a.t = table_of();
        HIPOK(hipMemsetAsync(&d_ctr.as<L2mCtr>()->overflow, 0, sizeof(unsigned int), st));
        if (!words.pass(f, st, "k_tsz_extract", [](Words &w) { memset(&w, 0, sizeof(w)); w.firsts[0] = ~0ull; }, [&] { launch_tsz_extract(a, st); })) return false;
        HIPOK(hipMemcpy(&hc, d_ctr.p, sizeof(hc), hipMemcpyDeviceToHost));
        if (hc.overflow) { if (!grow()) return false; continue; }         // no window was touched yet: the pass runs again
        if (hw.firsts[0] < a.n) {
            a.n = n = hw.firsts[0];
            if (n == 0) return true;
            continue;
        }
        break;
    }
    nids = hc.n_series;
    if (hw.counts[2]) { set_err("filter_throttle_size: a record is larger than 4 GB"); return false; }
    const uint64_t n_rec = hw.counts[0];
    uint64_t dropped = hw.counts[4];
    if (hw.counts[3]) {
        TszAdmitArgs ad;
        memset(&ad, 0, sizeof(ad));
        ad.w = windows_of(); ad.m = hw.counts[3]; ad.load = a.load; ad.len = a.len; ad.rate = cfg.rate;
        ad.now = now ? now : clock_now(); ad.wave_min = wave_min; ad.counts = dw->adm;
        // (one round trip of the counter words around three timed stretches: the order, the lanes' admission, the waves')
        hw.adm[0] = hw.adm[1] = 0;
        HIPOK(hipMemcpyAsync(dw, &hw, sizeof(hw), hipMemcpyHostToDevice, st));
        bool ordered;
        { ProfScope ps(f, st, "k_tsz_keys+sort"); ordered = launch_tsz_order(ad, a.wid, n, nids, d_work.p, d_work.cap, st); }
        if (!ordered) { (void) hipStreamSynchronize(st); set_err("filter_throttle_size: the sort by window failed"); return false; }
        { ProfScope ps(f, st, "k_tsz_admit<lane>"); launch_tsz_admit(ad, false, st); }
        { ProfScope ps(f, st, "k_tsz_admit<wave>"); launch_tsz_admit(ad, true, st); }
        HIPOK(hipMemcpyAsync(&hw, dw, sizeof(hw), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        dropped += hw.adm[0];
        created += hw.adm[1]; live += hw.adm[1];
    }
    n_in += n_rec; n_kept += n_rec - dropped; n_dropped += dropped; n_exempt += hw.counts[1];
    f->last_in = n_rec; f->last_out = n_rec - dropped;
    if (dropped == 0) return true;                                      // old_size == new_size (:719-722)
    if (!scan_lengths(f, st, a.len, n, &total)) return false;
    *ret = FLBGPU_FILTER_MODIFIED;
    if (total == 0) { memset(out, 0, sizeof(*out)); return true; }
    GatherArgs ga;
    ga.data = (const uint8_t *) in->data; ga.row_off = in->row_off; ga.n = n; ga.keep_len = a.len;
    ga.out_off = f->d_off.as<uint64_t>(); ga.out = f->d_out.as<uint8_t>(); ga.out_cap = 0;
    { ProfScope ps(f, st, "k_gather"); launch_gather(ga, st); }
    HIPOK(hipStreamSynchronize(st));
    set_out(f, out, n, total);
    return true;
}

// size_time_ticker's loop body (:175-186)
bool TszState::tick(flbgpu_filter *f, int64_t seconds) {
    std::lock_guard<std::mutex> lock(mu);
    if (!on_device()) return false;
    started = true;
    const int64_t ts = seconds ? seconds : clock_now();
    if (!words.ensure()) return false;
    TszTickArgs a;
    a.w = windows_of(); a.nids = nids; a.ts = ts;
    a.threshold = (long long) ((double) ts - (double) (long) cfg.duration);      // long time_treshold = current_timestamp - seconds (:125)
    a.counts = words.dev()->adm;
    if (!words.pass(f, f->stream, "k_tsz_tick", [](Words &w) { w.adm[0] = w.adm[1] = 0; }, [&] { launch_tsz_tick(a, f->stream); })) return false;
    live = words.host().adm[0];
    deleted += words.host().adm[1];
    return true;
}

bool TszState::view(flbgpu_tsz_windows *out) {
    std::lock_guard<std::mutex> lock(mu);
    if (!on_device()) return false;
    L2mCtr c;
    HIPOK(hipMemcpy(&c, d_ctr.p, sizeof(c), hipMemcpyDeviceToHost));
    clip(c);
    HostWindows h;
    if (!download(h, c.n_series, c.arena_used)) return false;
    const size_t W = cfg.window;
    v_names.clear(); v_name_off.assign(1, 0); v_total.clear(); v_ts.clear(); v_head.clear(); v_pane_size.clear(); v_pane_ts.clear();
    for (uint32_t i = 0; i < c.n_series; i++) {
        if (!h.exists[i]) continue;
        v_names.append((const char *) h.arena.data() + h.key_off[i], h.key_len[i]);
        v_name_off.push_back(v_names.size());
        v_total.push_back(h.total[i]); v_ts.push_back(h.timestamp[i]); v_head.push_back(h.head[i]);
        for (size_t p = 0; p < W; p++) { v_pane_size.push_back(h.pane_size[i * W + p]); v_pane_ts.push_back(h.pane_ts[i * W + p]); }
    }
    out->count = v_total.size(); out->window = cfg.window;
    out->names = v_names.data(); out->name_off = v_name_off.data(); out->total = v_total.data(); out->timestamp = v_ts.data();
    out->head = v_head.data(); out->pane_size = v_pane_size.data(); out->pane_ts = v_pane_ts.data();
    return true;
}

// ---- filter_throttle

struct ThrConfig {
    double rate = 1.0;
    uint32_t window = 5;
    int interval = 1;
};

// the config map (:301-328) and configure (:113-130); the interval as parse_duration (:132-154) answers it
bool thr_parse(int nprops, const char *const *names, const char *const *values, ThrConfig &c, std::string &why) {
    static const char *const known[] = {"rate", "window", "print_status", "interval"};
    int seen[4] = {0, 0, 0, 0};
    double rate = 1.0;
    int window = 5;
    std::string interval = "1";
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        if (val.find("${") != std::string::npos) { why = name + " '" + val + "': environment variables are not translated"; return false; }
        int k = -1;
        for (int j = 0; j < 4; j++) if (!strcasecmp(name.c_str(), known[j])) k = j;
        if (k < 0) { why = "unknown configuration property '" + name + "'"; return false; }
        if (++seen[k] > 1) { why = "configuration property '" + name + "' is set more than once"; return false; }
        if (k == 0) rate = atof(val.c_str());
        else if (k == 1) window = atoi(val.c_str());
        else if (k == 2) { if (utils_bool(val.c_str()) < 0) { why = "print_status '" + val + "': not a boolean"; return false; } }
        else interval = val;
    }
    c.rate = rate <= 1.0 ? 1.0 : rate;
    c.window = (unsigned int) window <= 1 ? 5u : (unsigned int) window;
    if (c.window > 65536) { why = "window '" + std::to_string(window) + "': more than 65536 panes"; return false; }
    char *p;
    double s = strtod(interval.c_str(), &p);
    if (!(0 >= s || (*p && *(p + 1)))) apply_suffix(&s, *p);             // (a bad interval is warned about and taken as it was read)
    if (!(s > -2147483649.0 && s < 2147483648.0)) { why = "interval '" + interval + "': more seconds than an int holds"; return false; }
    c.interval = (int) (0.0 + s);
    return true;
}

std::string thr_describe(const ThrConfig &c) {
    return "rate=" + fmt_g(c.rate) + ";window=" + std::to_string(c.window) + ";interval=" + std::to_string(c.interval);
}

struct ThrState : FilterState {
    struct Words { unsigned long long firsts[1], counts[5]; };
    struct Pane { long timestamp = 0, counter = 0; };
    std::mutex mu;
    ThrConfig cfg;
    // struct throttle_window (window.h:27-34)
    long current_timestamp = 0;
    unsigned total = 0;
    int max_index = -1;
    std::vector<Pane> table;
    uint64_t n_in = 0, n_kept = 0, n_dropped = 0;
    ScopedDevBuf d_table, d_wid, d_idx;
    CallWords<Words> words;
    void window_add(long timestamp, int val);
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

// window_add (window.c:69-97)
void ThrState::window_add(long timestamp, int val) {
    current_timestamp = timestamp;
    const int size = (int) table.size();
    int index = -1;
    for (int i = 0; i < size; i++) if (table[i].timestamp == timestamp) { index = i; break; }
    if (index < 0) {
        if (size - 1 == max_index) max_index = -1;
        max_index += 1;
        table[max_index].timestamp = timestamp;
        table[max_index].counter = val;
    }
    else table[index].counter += val;
    int sum = 0;
    for (int i = 0; i < size; i++) sum += (int) table[i].counter;
    total = (unsigned) sum;
}

// cb_throttle_filter (:190-272) on a device chunk: the records are found and counted on the device, K -- how many of them
// throttle_data (:101-111) keeps -- follows on the host from the reference's own comparison, record by record, and the rows behind
// the K-th record lose their length before the kept ones are copied.
bool ThrState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool) {
    std::lock_guard<std::mutex> lock(mu);
    uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0) return true;
    if (!words.ensure() || !ensure_row_columns(f, n) || !d_wid.ensure(n * 4) || !d_idx.ensure((n + 1) * 8)) return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    uint64_t &total_bytes = words.total();
    TszArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = TSZ_HDR_WORDS * 4; a.hash_mask = ~0ull;
    a.wid = d_wid.as<uint32_t>(); a.load = nullptr; a.len = f->d_len.as<uint32_t>();      // (no load: the rows are only told apart)
    a.firsts = dw->firsts; a.counts = dw->counts;
    for (;;) {
        if (!words.pass(f, st, "k_tsz_extract(records)", [](Words &w) { memset(&w, 0, sizeof(w)); w.firsts[0] = ~0ull; }, [&] { launch_tsz_extract(a, st); })) return false;
        if (hw.firsts[0] >= a.n) break;
        a.n = n = hw.firsts[0];
        if (n == 0) return true;
    }
    if (hw.counts[2]) { set_err("filter_throttle: a record is larger than 4 GB"); return false; }
    const uint64_t n_rec = hw.counts[0];
    uint64_t K = 0;
    size_t pane = 0;
    while (K < n_rec && !((total / (double) table.size()) >= cfg.rate)) {
        // (behind the call's first window_add its pane -- the first one of that timestamp, found once -- takes every further record
        // and the sum is the one before plus one)
        if (K == 0) {
            window_add(current_timestamp, 1);
            while (pane < table.size() && table[pane].timestamp != current_timestamp) pane++;
        }
        else { table[pane].counter += 1; total += 1; }
        K++;
    }
    n_in += n_rec; n_kept += K; n_dropped += n_rec - K;
    f->last_in = n_rec; f->last_out = K;
    if (K == n_rec) return true;
    *ret = FLBGPU_FILTER_MODIFIED;
    if (K == 0) { memset(out, 0, sizeof(*out)); return true; }
    { ProfScope ps(f, st, "k_scan"); launch_scan(a.wid, n, f->d_scan_tmp.as<uint64_t>(), d_idx.as<uint64_t>(), st, nullptr); }
    { ProfScope ps(f, st, "k_thr_first"); launch_thr_first(a.len, d_idx.as<uint64_t>(), K, n, st); }
    if (!scan_lengths(f, st, a.len, n, &total_bytes)) return false;
    GatherArgs ga;
    ga.data = (const uint8_t *) in->data; ga.row_off = in->row_off; ga.n = n; ga.keep_len = a.len;
    ga.out_off = f->d_off.as<uint64_t>(); ga.out = f->d_out.as<uint8_t>(); ga.out_cap = 0;
    { ProfScope ps(f, st, "k_gather"); launch_gather(ga, st); }
    HIPOK(hipStreamSynchronize(st));
    set_out(f, out, n, total_bytes);
    return true;
}

}  // namespace

extern "C" int flbgpu_throttle_size_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    TszConfig c;
    std::vector<uint32_t> table;
    if (!tsz_checked(nprops, names, values, c, table)) return -1;
    put_desc(desc, cap, tsz_describe(c));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_throttle_size_create(int nprops, const char *const *names, const char *const *values) {
    TszConfig c;
    std::vector<uint32_t> table;
    if (!tsz_checked(nprops, names, values, c, table)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_THROTTLE_SIZE;
    auto *m = new TszState();
    f->state = m;
    m->cfg = c;
    m->table_bytes = (uint32_t) (table.size() * 4);
    const uint64_t bits = env_u64("FLBGPU_TSZ_HASH_BITS", 64, 1, 64);
    m->hash_mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    m->wave_min = (uint32_t) env_u64("FLBGPU_TSZ_WAVE_MIN", TSZ_WAVE_MIN, 1, 0x7fffffff);
    uint64_t cap = 16;
    const uint64_t slots = env_u64("FLBGPU_TSZ_DICT_SLOTS", 1u << 16, 1, 1u << 30);
    while (cap < slots) cap <<= 1;
    // the panes take 16 bytes a pane and id: a large window starts with fewer ids (256 MiB of panes at most), and grows like any other
    while (cap > 16 && (cap / 2) * (uint64_t) c.window * 16 > ((uint64_t) 256 << 20)) cap >>= 1;
    m->cap = cap;
    (void) hipGetDevice(&m->device);
    m->arena_cap = std::max<uint64_t>(4096, cap * 32);
    HostWindows none;
    const bool star = c.name_parts.empty();
    if (!filter_common_init(f) || !upload(m->d_table, table) || !(star ? m->stamp_star(clock_now()) : m->rebuild(none, 0, m->cap, m->arena_cap))) {
        set_err("filter_throttle_size: the tables could not be placed on the device");
        delete f;
        return nullptr;
    }
    if (star) { m->live = 1; m->created = 1; }
    return f;
}

extern "C" int flbgpu_throttle_size_tick(flbgpu_filter *f, int64_t seconds) {
    TszState *m = state_of<TszState>(f, F_THROTTLE_SIZE);
    if (!m) { set_err("filter_throttle_size: not a throttle_size filter"); return -1; }
    return m->tick(f, seconds) ? 0 : -1;
}

extern "C" int flbgpu_throttle_size_set_now(flbgpu_filter *f, int64_t seconds) {
    TszState *m = state_of<TszState>(f, F_THROTTLE_SIZE);
    if (!m) { set_err("filter_throttle_size: not a throttle_size filter"); return -1; }
    std::lock_guard<std::mutex> lock(m->mu);
    m->now = seconds;
    if (!m->on_device()) return -1;
    if (!m->started && m->cfg.name_parts.empty() && !m->redate_star(seconds ? seconds : clock_now())) return -1;
    return 0;
}

extern "C" void flbgpu_throttle_size_counters(flbgpu_filter *f, uint64_t out[9]) {
    memset(out, 0, 9 * sizeof(uint64_t));
    if (auto *m = state_of<TszState>(f, F_THROTTLE_SIZE)) {
        std::lock_guard<std::mutex> lock(m->mu);
        out[0] = m->n_in; out[1] = m->n_kept; out[2] = m->n_dropped; out[3] = m->n_exempt; out[4] = m->live; out[5] = m->created;
        out[6] = m->deleted; out[7] = m->grows; out[8] = m->nids;
    }
}

extern "C" int flbgpu_throttle_size_windows(flbgpu_filter *f, flbgpu_tsz_windows *out) {
    if (!out) return -1;
    memset(out, 0, sizeof(*out));
    TszState *m = state_of<TszState>(f, F_THROTTLE_SIZE);
    if (!m) { set_err("filter_throttle_size: not a throttle_size filter"); return -1; }
    return m->view(out) ? 0 : -1;
}

extern "C" int flbgpu_throttle_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    ThrConfig c;
    if (!parse_front("throttle", nprops, names, values, [&](std::string &why) { return thr_parse(nprops, names, values, c, why); })) return -1;
    put_desc(desc, cap, thr_describe(c));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_throttle_create(int nprops, const char *const *names, const char *const *values) {
    ThrConfig c;
    if (!parse_front("throttle", nprops, names, values, [&](std::string &why) { return thr_parse(nprops, names, values, c, why); })) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_THROTTLE;
    auto *m = new ThrState();
    f->state = m;
    m->cfg = c;
    m->table.assign(c.window, ThrState::Pane());
    const std::vector<uint32_t> table(TSZ_HDR_WORDS, 0);                 // no paths: every record is `*`'s
    if (!filter_common_init(f) || !upload(m->d_table, table)) {
        set_err("filter_throttle: the filter could not be placed on the device");
        delete f;
        return nullptr;
    }
    return f;
}

extern "C" int flbgpu_throttle_tick(flbgpu_filter *f, int64_t seconds) {
    ThrState *m = state_of<ThrState>(f, F_THROTTLE);
    if (!m) { set_err("filter_throttle: not a throttle filter"); return -1; }
    std::lock_guard<std::mutex> lock(m->mu);
    const long ts = seconds ? (long) seconds : (long) clock_now();
    m->window_add(ts, 0);
    m->current_timestamp = ts;
    return 0;
}

extern "C" void flbgpu_throttle_counters(flbgpu_filter *f, uint64_t out[3]) {
    out[0] = out[1] = out[2] = 0;
    if (auto *m = state_of<ThrState>(f, F_THROTTLE)) {
        std::lock_guard<std::mutex> lock(m->mu);
        out[0] = m->n_in; out[1] = m->n_kept; out[2] = m->n_dropped;
    }
}
