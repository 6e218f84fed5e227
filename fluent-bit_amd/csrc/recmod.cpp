// recmod.cpp -- filter_record_modifier (plugins/filter_record_modifier/filter_modifier.c): the configuration as configure() reads it
// (:69-155, behind the config map of :499-529), the device program behind it, and one cb_modifier_filter call on a device chunk
// (:298-486).  The per-record work is recmod_kernels.inc.
#include "filter_host.hpp"
#include "recmod.hpp"

using namespace flbgpu;

// token_retrieve (src/flb_slist.c:107-180): one token of a line; *pos < 0 when the line has ended.  false: no token.
static bool next_token(const std::string &s, long *pos, std::string &tok) {
    if (*pos < 0) return false;
    const char *b = s.c_str();
    const char *p = b + *pos;
    while (*p == ' ') p++;
    const char *start = p;
    bool quoted = false;
    if (*p == '"') {
        quoted = true;
        start = ++p;
        for (;;) {
            while (*p && *p != '"') p++;
            if (!*p) break;
            if (p[-1] == '\\') { p++; continue; }       // an escaped quote (the byte in front of the opening quote counts too)
            break;
        }
    }
    else while (*p && *p != ' ') p++;
    if (*p) {                                           // (a closed quote ends the token where the quote stands)
        tok.assign(start, (size_t) (p - start));
        if (quoted) {
            // token_unescape: \" -> "
            std::string u;
            for (size_t i = 0; i < tok.size();) {
                if (tok[i] == '\\' && i + 1 < tok.size() && tok[i + 1] == '"') { u.push_back('"'); i += 2; }
                else u.push_back(tok[i++]);
            }
            tok = u;
        }
        p++;
        while (*p == ' ') p++;
        *pos = (long) (p - b);
        return true;
    }
    *pos = -1;
    if (p > start) { tok.assign(start); return true; }  // the rest of the line (an unterminated quote keeps its text as it is)
    return false;
}

// flb_slist_split_tokens(list, str, max) (src/flb_slist.c:182-217): `max` tokens, then the rest of the line as one more entry
void flbgpu::slist_split_tokens(const std::string &s, int max, std::vector<std::string> &out) {
    out.clear();
    long pos = 0;
    int count = 0;
    std::string tok;
    while (next_token(s, &pos, tok)) {
        out.push_back(tok);
        if (pos < 0) break;
        if (++count >= max) {
            const char *p = s.c_str() + pos;
            while (*p == ' ') p++;
            if (*p) out.emplace_back(p);
            break;
        }
    }
}

namespace {

struct RKey { std::string key; bool prefix; };
struct RProgram {
    int list = RECMOD_NONE;
    std::vector<RKey> keys;
    std::vector<std::pair<std::string, std::string>> records;
};

// the config map (:499-529) and configure() (:69-155) over the properties in configuration order
bool parse_program(int nprops, const char *const *names, const char *const *values, RProgram &pg, std::string &why) {
    std::vector<RKey> remove, allow, white;
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        if (!strcasecmp(name.c_str(), "record")) {
            std::vector<std::string> tok;
            slist_split_tokens(val, 2, tok);
            // SLIST_2: fewer than two entries fail the config map's size check (src/flb_config_map.c:32-59) and the filter does not
            // start; more than two pass it and configure() skips the entry with a message (:96-101)
            if (tok.size() < 2) { why = "Record needs 'KEY VALUE': " + val; return false; }
            if (tok.size() > 2) continue;
            pg.records.emplace_back(tok[0], tok[1]);
            if ((int) pg.records.size() > RECMOD_MAX_RECORDS) { why = "more than " + std::to_string(RECMOD_MAX_RECORDS) + " Record entries"; return false; }
            continue;
        }
        std::vector<RKey> *dst = nullptr;
        if (!strcasecmp(name.c_str(), "remove_key")) dst = &remove;
        else if (!strcasecmp(name.c_str(), "allowlist_key")) dst = &allow;
        else if (!strcasecmp(name.c_str(), "whitelist_key")) dst = &white;
        else if (!strcasecmp(name.c_str(), "uuid_key")) { why = "Uuid_key is not supported: its value is random per record"; return false; }
        else { why = "unknown configuration property '" + name + "'"; return false; }
        // (the reference reads key[-1] of an empty key, :56 and :134)
        if (val.empty()) { why = name + " with an empty key"; return false; }
        RKey k;
        k.prefix = val.back() == '*';
        k.key = k.prefix ? val.substr(0, val.size() - 1) : val;
        dst->push_back(k);
    }
    // Whitelist_key joins the allowlist behind the Allowlist_key entries (:146-147)
    allow.insert(allow.end(), white.begin(), white.end());
    if (!remove.empty() && !allow.empty()) { why = "remove_keys and allowlist_keys are exclusive with each other"; return false; }
    pg.list = !remove.empty() ? RECMOD_REMOVE : !allow.empty() ? RECMOD_ALLOW : RECMOD_NONE;
    pg.keys = !remove.empty() ? remove : allow;
    if ((int) pg.keys.size() > RECMOD_MAX_KEYS) { why = "more than " + std::to_string(RECMOD_MAX_KEYS) + " key entries"; return false; }
    size_t bytes = 0;
    for (const RKey &k : pg.keys) bytes += (k.key.size() + 3) & ~(size_t) 3;
    if (bytes > RECMOD_MAX_KEY_BYTES) { why = "key entries longer than " + std::to_string(RECMOD_MAX_KEY_BYTES) + " bytes together"; return false; }
    return true;
}

std::string describe(const RProgram &pg) {
    std::string d = pg.list == RECMOD_REMOVE ? "remove" : pg.list == RECMOD_ALLOW ? "allow" : "none";
    for (const RKey &k : pg.keys) d += std::string(";K") + (k.prefix ? "p" : "e") + "," + hexs(k.key);
    for (const auto &r : pg.records) d += ";R" + hexs(r.first) + "," + hexs(r.second);
    return d;
}

void pack_str(std::vector<uint8_t> &o, const std::string &s) {
    const size_t n = s.size();
    if (n < 32) o.push_back((uint8_t) (0xa0 | n));
    else if (n < 256) { o.push_back(0xd9); o.push_back((uint8_t) n); }
    else if (n < 65536) { o.push_back(0xda); o.push_back((uint8_t) (n >> 8)); o.push_back((uint8_t) n); }
    else { o.push_back(0xdb); for (int i = 3; i >= 0; i--) o.push_back((uint8_t) (n >> (8 * i))); }
    o.insert(o.end(), s.begin(), s.end());
}

bool front(int nprops, const char *const *names, const char *const *values, RProgram &pg) {
    return parse_front("record_modifier", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, pg, why); });
}

struct RecmodState : FilterState {
    struct Words { unsigned long long first_bad, first_wide, counts[4]; };
    int list = RECMOD_NONE, nkeys = 0;
    uint32_t nrec = 0, table_bytes = 0, tail_len = 0;
    ScopedDevBuf d_table, d_tail;
    CallWords<Words> words;
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

}  // namespace

extern "C" int flbgpu_record_modifier_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    RProgram pg;
    if (!front(nprops, names, values, pg)) return -1;
    put_desc(desc, cap, describe(pg));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_record_modifier_create(int nprops, const char *const *names, const char *const *values) {
    RProgram pg;
    if (!front(nprops, names, values, pg)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_RECMOD;
    auto *m = new RecmodState();
    f->state = m;
    m->list = pg.list;
    m->nkeys = (int) pg.keys.size();
    m->nrec = (uint32_t) pg.records.size();
    // the key table (recmod.hpp): lengths and offsets, then the bytes folded as tolower does in the C locale
    std::vector<uint32_t> table(2 * pg.keys.size());
    for (size_t i = 0; i < pg.keys.size(); i++) {
        const std::string &k = pg.keys[i].key;
        table[2 * i] = (uint32_t) k.size() | (pg.keys[i].prefix ? RECMOD_PREFIX : 0u);
        table[2 * i + 1] = (uint32_t) (table.size() * 4);
        for (size_t j = 0; j < k.size(); j += 4) {
            uint32_t w = 0;
            for (size_t b = 0; b < 4 && j + b < k.size(); b++) {
                unsigned char c = (unsigned char) k[j + b];
                if (c >= 'A' && c <= 'Z') c |= 0x20;
                w |= (uint32_t) c << (8 * b);
            }
            table.push_back(w);
        }
    }
    m->table_bytes = (uint32_t) (table.size() * 4);
    std::vector<uint8_t> tail;
    for (const auto &r : pg.records) { pack_str(tail, r.first); pack_str(tail, r.second); }
    m->tail_len = (uint32_t) tail.size();
    if (!filter_common_init(f) || !upload(m->d_table, table) || !upload(m->d_tail, tail)) { delete f; return nullptr; }
    return f;
}

// cb_modifier_filter (:298-486) on a device chunk.  A decoder error ends the loop and the call answers with what was encoded in
// front of it (:351-353, :469-477) -- so undecodable bytes behind the rows (`garbage`) change nothing here.
bool RecmodState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool) {
    const uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0) return true;
    if (!words.ensure() || !ensure_row_columns(f, n)) return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    RecmodArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = table_bytes; a.nkeys = nkeys; a.list = list;
    a.nrec = nrec; a.tail = d_tail.as<uint8_t>(); a.tail_len = tail_len;
    a.len = f->d_len.as<uint32_t>();
    a.first_bad = &dw->first_bad; a.first_wide = &dw->first_wide; a.counts = dw->counts;
    auto size_pass = [&](const char *name) {
        return words.pass(f, st, name, [](Words &w) { memset(&w, 0, sizeof(w)); w.first_bad = ~0ull; w.first_wide = ~0ull; }, [&] { launch_recmod(a, false, st); });
    };
    if (!size_pass("k_recmod(size)")) return false;
    const unsigned long long fb = hw.first_bad;
    // a body of more than 65535 entries that the loop reaches: the call gives up with -1 and nothing emitted (:369-377)
    if (hw.first_wide != ~0ull && hw.first_wide < fb) {
        set_err("filter_record_modifier: The number of elements exceeds limit 65535");
        *ret = -1;
        return true;
    }
    if (fb == 0) return true;
    if (fb != ~0ull) {
        // the loop ends at the first record the decoder refuses: the call is the rows in front of it -- nothing is emitted for the
        // others, and the call-level facts are counted again over those rows only
        HIPOK(hipMemsetAsync(a.len + fb, 0, (n - fb) * sizeof(uint32_t), st));
        a.n = fb;
        if (!size_pass("k_recmod(size, in front of a decoder error)")) return false;
    }
    if (hw.counts[3]) { set_err("filter_record_modifier: a record's output is larger than 4 GB"); return false; }
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[0];
    // is_modified: a key was removed somewhere, or Record entries were appended to a record; MODIFIED needs a byte in the encoder too
    const bool is_modified = hw.counts[2] > 0 || (nrec > 0 && hw.counts[0] > 0);
    if (!is_modified || hw.counts[1] == 0) return true;
    const uint64_t n_out = hw.counts[1];
    if (!scan_lengths(f, st, a.len, n, &words.total())) return false;
    a.out_off = f->d_off.as<uint64_t>(); a.out = f->d_out.as<uint8_t>();
    { ProfScope ps(f, st, "k_recmod(emit)"); launch_recmod(a, true, st); }
    HIPOK(hipStreamSynchronize(st));
    set_out(f, out, n, words.total());
    f->last_out = n_out;
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
