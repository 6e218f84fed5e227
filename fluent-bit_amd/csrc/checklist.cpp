// checklist.cpp -- filter_checklist (plugins/filter_checklist/checklist.c): the configuration as the config map (:601-640) and
// init_config (:198-267) read it, the list loader (load_file_patterns :130-196) restated over the file's bytes, the lookup
// structures for HBM (an open-addressed table for mode exact, first-byte buckets for mode partial), and one cb_checklist_filter
// call on a device chunk (:411-582).  The per-record work is checklist_kernels.inc.
#include "filter_host.hpp"
#include "checklist.hpp"

using namespace flbgpu;

namespace {

enum { LOAD_OK = 0, LOAD_NO_FILE = 1, LOAD_CANNOT_OPEN = 2, LOAD_STOPPED = 3 };

struct CProgram {
    int mode = CL_EXACT, fold = 0;
    bool inert = false;                  // the accessor has no key part: nothing is ever found
    DevKey key;
    std::vector<std::pair<std::string, std::string>> recs;
    bool has_file = false;
    std::string file;
    int load = LOAD_OK, stop_line = 0;
    std::vector<std::string> entries;    // in file order, as they were added (folded when ignore_case is set)
};

// flb_utils_bool (src/flb_utils.c:757-771)
int bool_of(const std::string &v) {
    if (!strcasecmp(v.c_str(), "true") || !strcasecmp(v.c_str(), "on") || !strcasecmp(v.c_str(), "yes")) return 1;
    if (!strcasecmp(v.c_str(), "false") || !strcasecmp(v.c_str(), "off") || !strcasecmp(v.c_str(), "no")) return 0;
    return -1;
}

int value_kind(const std::string &v) {                 // set_record (:379-393): strcasecmp on the whole value
    if (!strcasecmp(v.c_str(), "true")) return CL_VAL_TRUE;
    if (!strcasecmp(v.c_str(), "false")) return CL_VAL_FALSE;
    if (!strcasecmp(v.c_str(), "null")) return CL_VAL_NIL;
    return CL_VAL_STR;
}

// load_file_patterns (:130-196) over the bytes of the file: fgets(buf, 2047) takes at most 2046 bytes and stops behind a '\n'; the
// end-of-file mark is set only by a read that ran out of bytes.  false: a piece begins with a NUL byte (the reference reads buf[-1])
bool load_list(const std::string &d, int fold, CProgram &pg, std::string &why) {
    size_t pos = 0;
    int line = 0;
    while (pos < d.size()) {
        size_t take = 0;
        bool nl = false;
        while (take < CL_LINE - 2 && pos + take < d.size()) { const char c = d[pos + take++]; if (c == '\n') { nl = true; break; } }
        const bool eof = !nl && take < CL_LINE - 2;
        size_t len = strnlen(d.data() + pos, take);
        const char *b = d.data() + pos;
        pos += take;
        if (len == 0) { why = "the list has a NUL byte at the start of a line (the reference reads out of bounds there)"; return false; }
        if (b[len - 1] == '\n') { len--; if (len && b[len - 1] == '\r') len--; }
        else if (!eof) { pg.load = LOAD_STOPPED; pg.stop_line = line; return true; }
        if (len == 0 || b[0] == '#') { line++; continue; }
        std::string e(b, len);
        if (fold) for (char &c : e) if (c >= 'A' && c <= 'Z') c = (char) (c + 32);      // tolower in the C locale
        pg.entries.push_back(e);
        line++;
    }
    return true;
}

bool read_file(const std::string &path, std::string &out) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return false;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}

// the config map (:601-640) and init_config (:198-267)
bool parse_program(int nprops, const char *const *names, const char *const *values, CProgram &pg, std::string &why) {
    std::string lookup = "log", mode;
    bool have_mode = false;
    static const char *const once[] = {"file", "lookup_key", "mode", "ignore_case", "print_query_time"};
    int seen[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        const char *n = name.c_str();
        // a property without FLB_CONFIG_MAP_MULT that is set more than once fails the check of the properties (src/flb_config_map.c:551-560)
        for (int k = 0; k < 5; k++)
            if (!strcasecmp(n, once[k]) && ++seen[k] > 1) { why = "configuration property '" + name + "' is set more than once"; return false; }
        if (!strcasecmp(n, "file")) { pg.has_file = true; pg.file = val; }
        else if (!strcasecmp(n, "lookup_key")) lookup = val;
        else if (!strcasecmp(n, "mode")) { have_mode = true; mode = val; }
        else if (!strcasecmp(n, "ignore_case") || !strcasecmp(n, "print_query_time")) {
            const int b = bool_of(val);
            if (b < 0) { why = "invalid value for boolean property '" + name + "': " + val; return false; }
            if (!strcasecmp(n, "ignore_case")) pg.fold = b;
        }
        else if (!strcasecmp(n, "record")) {
            std::vector<std::string> tok;
            slist_split_tokens(val, 2, tok);
            // SLIST_2: fewer than two entries fail the config map's size check; what is behind the key is one entry
            if (tok.size() < 2) { why = "record needs 'KEY VALUE': " + val; return false; }
            pg.recs.emplace_back(tok.front(), tok.back());
        }
        else { why = "unknown configuration property '" + name + "'"; return false; }
    }
    if ((int) pg.recs.size() > CL_MAX_RECORDS) { why = "more than " + std::to_string(CL_MAX_RECORDS) + " record entries"; return false; }
    pg.mode = have_mode && !strcasecmp(mode.c_str(), "partial") ? CL_PARTIAL : CL_EXACT;
    // flb_ra_create(lookup_key, FLB_TRUE): the first part decides (get_ra_parser)
    if (lookup.find("${") != std::string::npos) { why = "lookup_key '" + lookup + "': environment variables are not translated"; return false; }
    std::vector<RaPart> parts;
    const int rc = ra_split(lookup, parts, why);
    if (!parts.empty() && parts[0].kind == RA_STR && parts[0].str.size() >= (size_t) MAX_KEY) {
        why = "lookup_key '" + lookup + "': key longer than " + std::to_string(MAX_KEY - 1) + " bytes";
        return false;
    }
    if (rc == RA_SPLIT_SKIP) { why = "lookup_key '" + lookup + "': the record accessor refuses it (the reference goes on with a NULL accessor)"; return false; }
    if (rc == RA_SPLIT_REFUSE) { why = "lookup_key '" + lookup + "': " + why; return false; }
    memset(&pg.key, 0, sizeof(pg.key));
    if (parts.empty() || (parts[0].kind != RA_STR && parts[0].kind != RA_KEY)) pg.inert = true;
    else if (parts[0].kind == RA_KEY) pg.key = parts[0].key;
    else {
        pg.key.is_ra = 1;
        memcpy(pg.key.key, parts[0].str.data(), parts[0].str.size());
        pg.key.key_len = (int) parts[0].str.size();
    }
    if (!pg.has_file) { pg.load = LOAD_NO_FILE; return true; }
    std::string bytes;
    if (!read_file(pg.file, bytes)) { pg.load = LOAD_CANNOT_OPEN; return true; }
    return load_list(bytes, pg.fold, pg, why);
}

void put_bytes(std::vector<uint32_t> &table, const char *s, size_t n) {
    for (size_t j = 0; j < n; j += 4) {
        uint32_t w = 0;
        for (size_t b = 0; b < 4 && j + b < n; b++) w |= (uint32_t) (unsigned char) s[j + b] << (8 * b);
        table.push_back(w);
    }
}

std::string packed_str(const std::string &s) {
    std::string o;
    const size_t n = s.size();
    if (n < 32) o.push_back((char) (0xa0 | n));
    else if (n < 256) { o.push_back((char) 0xd9); o.push_back((char) n); }
    else if (n < 65536) { o.push_back((char) 0xda); o.push_back((char) (n >> 8)); o.push_back((char) n); }
    else { o.push_back((char) 0xdb); for (int i = 3; i >= 0; i--) o.push_back((char) (n >> (8 * i))); }
    return o + s;
}

// the LDS table of checklist.hpp
void build_table(const CProgram &pg, std::vector<uint32_t> &table) {
    const size_t nrec = pg.recs.size();
    table.assign(CL_HDR_WORDS + CL_REC_WORDS * nrec, 0);
    const size_t sub = table.size();
    table.resize(sub + 2 * (size_t) pg.key.nsub, 0);
    for (int s = 0; s < pg.key.nsub; s++) {
        if (pg.key.sub_is_index[s]) { table[sub + 2 * s] = (uint32_t) pg.key.sub_index[s] | TC_SUB_INDEX; continue; }
        table[sub + 2 * s] = (uint32_t) pg.key.sub_len[s];
        table[sub + 2 * s + 1] = (uint32_t) (table.size() * 4);
        put_bytes(table, pg.key.sub_str + pg.key.sub_off[s], (size_t) pg.key.sub_len[s]);
    }
    table[0] = (uint32_t) nrec;
    table[1] = (uint32_t) pg.key.key_len | ((uint32_t) pg.key.nsub << 16) | (pg.inert ? CL_ACC_INERT : 0u);
    table[2] = (uint32_t) (table.size() * 4);
    table[3] = (uint32_t) (sub * 4);
    put_bytes(table, pg.key.key, (size_t) pg.key.key_len);
    for (size_t i = 0; i < nrec; i++) {
        const std::string &k = pg.recs[i].first, &v = pg.recs[i].second;
        std::string out = packed_str(k);
        switch (value_kind(v)) {
        case CL_VAL_TRUE: out.push_back((char) 0xc3); break;
        case CL_VAL_FALSE: out.push_back((char) 0xc2); break;
        case CL_VAL_NIL: out.push_back((char) 0xc0); break;
        default: out += packed_str(v); break;
        }
        const uint32_t koff = (uint32_t) (table.size() * 4);
        put_bytes(table, k.data(), k.size());
        const uint32_t ooff = (uint32_t) (table.size() * 4);
        put_bytes(table, out.data(), out.size());
        uint32_t *w = &table[CL_HDR_WORDS + CL_REC_WORDS * i];
        w[0] = (uint32_t) k.size(); w[1] = koff; w[2] = (uint32_t) out.size(); w[3] = ooff;
    }
}

uint64_t fnv1a(const uint8_t *p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// entries in order: 4 bytes of length (little endian), then the bytes
uint64_t digest(const CProgram &pg) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (const std::string &e : pg.entries) {
        uint8_t l[4];
        for (int i = 0; i < 4; i++) l[i] = (uint8_t) (e.size() >> (8 * i));
        h = fnv1a(l, 4, h);
        h = fnv1a((const uint8_t *) e.data(), e.size(), h);
    }
    return h;
}

// mode exact: the number of slots, a power of two: load factor <= 1/2, or -- the test switch FLBGPU_CHECKLIST_DENSE=1 -- the smallest
// power of two above the number of entries
uint32_t slot_count(const CProgram &pg) {
    if (pg.mode != CL_EXACT) return 0;
    const char *dense = getenv("FLBGPU_CHECKLIST_DENSE");
    const uint64_t want = dense && dense[0] == '1' ? (uint64_t) pg.entries.size() + 1 : 2 * (uint64_t) pg.entries.size();
    uint64_t ns = 1;
    while (ns < want) ns <<= 1;
    return (uint32_t) ns;
}

std::string describe(const CProgram &pg) {
    std::string d = std::string("mode=") + (pg.mode == CL_PARTIAL ? "partial" : "exact") + ";fold=" + (pg.fold ? "1" : "0") + ";key=";
    if (pg.inert) d += "-";
    else {
        d += "K" + hexs(std::string(pg.key.key, (size_t) pg.key.key_len));
        for (int s = 0; s < pg.key.nsub; s++) {
            if (pg.key.sub_is_index[s]) d += "[" + std::to_string(pg.key.sub_index[s]) + "]";
            else d += "." + hexs(std::string(pg.key.sub_str + pg.key.sub_off[s], (size_t) pg.key.sub_len[s]));
        }
    }
    d += ";records=";
    for (size_t i = 0; i < pg.recs.size(); i++) {
        static const char *const kinds[] = {"s", "t", "f", "n"};
        const int k = value_kind(pg.recs[i].second);
        d += (i ? "," : "") + ("K" + hexs(pg.recs[i].first)) + ":" + kinds[k] + (k == CL_VAL_STR ? hexs(pg.recs[i].second) : "");
    }
    d += ";entries=" + std::to_string(pg.entries.size()) + ";slots=" + std::to_string(slot_count(pg)) + ";load=";
    switch (pg.load) {
    case LOAD_NO_FILE: d += "no file"; break;
    case LOAD_CANNOT_OPEN: d += "cannot open"; break;
    case LOAD_STOPPED: d += "stopped at line " + std::to_string(pg.stop_line); break;
    default: d += "ok"; break;
    }
    char hx[32];
    snprintf(hx, sizeof(hx), "%016llx", (unsigned long long) digest(pg));
    return d + ";digest=" + hx;
}

bool checked_program(int nprops, const char *const *names, const char *const *values, CProgram &pg, std::vector<uint32_t> &table) {
    if (!parse_front("checklist", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, pg, why); })) return false;
    build_table(pg, table);
    if (table.size() * 4 > CL_MAX_TABLE_BYTES) { set_err("filter_checklist: record / accessor table larger than %u bytes", CL_MAX_TABLE_BYTES); return false; }
    uint64_t arena = 0;
    for (const std::string &e : pg.entries) arena += e.size();
    if (arena > 0xFFFFFF00ull || pg.entries.size() > 0x3FFFFFFFull) { set_err("filter_checklist: the list does not fit 32-bit offsets"); return false; }
    return true;
}

struct ChecklistState : FilterState {
    struct Words { unsigned long long firsts[5], counts[7]; };
    int mode = 0, fold = 0;
    uint32_t table_bytes = 0, arena_bytes = 0, nslots = 0, nents = 0;
    uint64_t matched = 0, rolled = 0, nonstr = 0, mismatch = 0;        // since the filter was created (flbgpu_checklist_counters)
    ScopedDevBuf d_table, d_arena, d_slots, d_bucket, d_ents, d_flags, d_enc;
    CallWords<Words> words;
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

}  // namespace

extern "C" int flbgpu_checklist_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    CProgram pg;
    std::vector<uint32_t> table;
    if (!checked_program(nprops, names, values, pg, table)) return -1;
    put_desc(desc, cap, describe(pg));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_checklist_create(int nprops, const char *const *names, const char *const *values) {
    CProgram pg;
    std::vector<uint32_t> table;
    if (!checked_program(nprops, names, values, pg, table)) return nullptr;
    // the arena: every distinct entry once, in order of first appearance
    std::string arena;
    std::vector<uint32_t> slots, bucket(CL_BUCKETS + 1, 0), ents;
    uint32_t nslots = 0;
    if (pg.mode == CL_EXACT) {
        // open addressing, linear probing, the hash of l2m's group dictionary (FNV-1a, 64 bits)
        nslots = slot_count(pg);
        slots.assign(4 * (size_t) nslots, 0);
        for (uint32_t s = 0; s < nslots; s++) slots[4 * (size_t) s + 2] = CL_EMPTY;
        for (const std::string &e : pg.entries) {
            const uint64_t h = fnv1a((const uint8_t *) e.data(), e.size());
            uint32_t pos = (uint32_t) h & (nslots - 1);
            bool dup = false;
            while (slots[4 * (size_t) pos + 2] != CL_EMPTY) {
                const uint32_t *w = &slots[4 * (size_t) pos];
                if (w[0] == (uint32_t) h && w[1] == (uint32_t) (h >> 32) && w[3] == e.size() && !memcmp(arena.data() + w[2], e.data(), e.size())) { dup = true; break; }
                pos = (pos + 1) & (nslots - 1);
            }
            if (dup) continue;
            uint32_t *w = &slots[4 * (size_t) pos];
            w[0] = (uint32_t) h; w[1] = (uint32_t) (h >> 32); w[2] = (uint32_t) arena.size(); w[3] = (uint32_t) e.size();
            arena += e;
        }
    }
    else {
        // one bucket per ASCII first byte that is a literal; `any`: entries that begin with '%', '_' or a byte >= 0x80
        auto bucket_of = [](const std::string &e) { const unsigned char c = (unsigned char) e[0]; return c == '%' || c == '_' || c >= 0x80 ? 256u : (uint32_t) c; };
        for (const std::string &e : pg.entries) bucket[bucket_of(e) + 1]++;
        for (uint32_t b = 0; b < CL_BUCKETS; b++) bucket[b + 1] += bucket[b];
        ents.assign(2 * pg.entries.size(), 0);
        std::vector<uint32_t> fill(bucket.begin(), bucket.end() - 1);
        for (const std::string &e : pg.entries) {
            const uint32_t at = fill[bucket_of(e)]++;
            ents[2 * (size_t) at] = (uint32_t) arena.size(); ents[2 * (size_t) at + 1] = (uint32_t) e.size();
            arena += e;
        }
    }
    auto *f = new flbgpu_filter();
    f->kind = F_CHECKLIST;
    auto *m = new ChecklistState();
    f->state = m;
    m->mode = pg.mode; m->fold = pg.fold;
    m->table_bytes = (uint32_t) (table.size() * 4);
    m->arena_bytes = (uint32_t) arena.size();
    m->nslots = nslots;
    m->nents = (uint32_t) (ents.size() / 2);
    if (!filter_common_init(f) || !upload(m->d_table, table) || !upload(m->d_arena, arena.data(), arena.size()) ||
        !upload(m->d_slots, slots) || !upload(m->d_bucket, bucket) || !upload(m->d_ents, ents)) {
        set_err("filter_checklist: the list could not be placed on the device");
        delete f;
        return nullptr;
    }
    return f;
}

extern "C" void flbgpu_checklist_counters(flbgpu_filter *f, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (auto *m = state_of<ChecklistState>(f, F_CHECKLIST)) { out[0] = m->matched; out[1] = m->rolled; out[2] = m->nonstr; out[3] = m->mismatch; }
}

// cb_checklist_filter (:411-582) on a device chunk.  The loop ends at the first record the decoder refuses; what stands behind it,
// and undecodable bytes behind the rows, are dropped from a MODIFIED answer and change nothing else.
bool ChecklistState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool) {
    uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0) return true;
    if (!words.ensure() || !ensure_row_columns(f, n) || !d_enc.ensure(n * sizeof(uint32_t)) || !d_flags.ensure(n)) return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    uint64_t &total = words.total();
    ChecklistArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = table_bytes;
    a.mode = mode; a.fold = fold;
    a.arena = d_arena.as<uint8_t>(); a.arena_bytes = arena_bytes;
    a.slots = d_slots.as<uint32_t>(); a.nslots = nslots;
    a.bucket_off = d_bucket.as<uint32_t>(); a.ents = d_ents.as<uint32_t>(); a.nents = nents;
    a.flags = d_flags.as<uint8_t>(); a.enc_len = d_enc.as<uint32_t>(); a.len = f->d_len.as<uint32_t>();
    a.firsts = dw->firsts; a.counts = dw->counts;
    auto size_pass = [&](const char *name) {
        return words.pass(f, st, name, [](Words &w) { memset(w.firsts, 0xff, sizeof(w.firsts)); memset(w.counts, 0, sizeof(w.counts)); },
                          [&] { launch_checklist(a, false, st); });
    };
    if (!size_pass("k_checklist(size)")) return false;
    const unsigned long long fb = hw.firsts[0];
    if (fb == 0) return true;
    if (fb != ~0ull) {
        // the loop ends at the first record the decoder refuses: the call is the rows in front of it
        a.n = n = fb;
        if (!size_pass("k_checklist(size, in front of a decoder error)")) return false;
    }
    matched += hw.counts[2]; rolled += hw.counts[3]; nonstr += hw.counts[4];
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[0];
    if (hw.counts[5]) { set_err("filter_checklist: a record's output is larger than 4 GB"); return false; }
    if (hw.counts[2] == 0) return true;                                  // matches == 0 (:566-578)
    // the first match that leaves something in the output: the first one, unless it is the first record of the chunk AND the encoder
    // refused it -- then output_length is still 0 and the next match emits everything in front of it as one raw span (:541-547)
    unsigned long long eff = hw.firsts[2];
    if (hw.firsts[2] == hw.firsts[1] && hw.firsts[3] != hw.firsts[2]) {
        a.after = hw.firsts[2];
        { ProfScope ps(f, st, "k_checklist_second"); launch_checklist_second(a, st); }
        HIPOK(hipMemcpyAsync(&hw.firsts[4], &dw->firsts[4], sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        eff = hw.firsts[4];
        if (eff == ~0ull) return true;                                   // output_length stayed 0 (:566)
    }
    a.first_eff = eff;
    { ProfScope ps(f, st, "k_checklist_plan"); launch_checklist_plan(a, st); }
    // (the records in the encoder come over in the scan's sync)
    if (!scan_lengths_queue(f, st, a.len, n, &total)) return false;
    HIPOK(hipMemcpyAsync(&hw.counts[1], &dw->counts[1], sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (!scan_lengths_wait(f, st, &total)) return false;
    if (total == 0) return true;                                         // (a first record that matched, was refused, and nothing else)
    a.out_off = f->d_off.as<uint64_t>(); a.out = f->d_out.as<uint8_t>();
    { ProfScope ps(f, st, "k_checklist(emit)"); launch_checklist(a, true, st); }
    HIPOK(hipMemcpyAsync(&hw.counts[6], &dw->counts[6], sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    mismatch += hw.counts[6];
    if (hw.counts[6]) { set_err("filter_checklist: %llu rows were emitted with another length than they were sized", hw.counts[6]); return false; }
    set_out(f, out, n, total);
    f->last_out = hw.counts[1];
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
