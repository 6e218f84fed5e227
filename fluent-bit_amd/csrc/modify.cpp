// modify.cpp -- filter_modify (plugins/filter_modify/modify.c): the configuration as setup() reads it (:141-519), the device
// program behind it, and one cb_modify_filter call on a device chunk (:1486-1578).  The per-record work is modify_kernels.inc.
#include "filter_host.hpp"
#include "mod.hpp"

using namespace flbgpu;

namespace {

// flb_utils_split_quoted(val, ' ', 3) (src/flb_utils.c:278-462): quoted tokens with \" \' \\ inside, leading separators skipped, the
// empty token of a line that ends in separators, a 4th entry with the rest of the line.  false: an unterminated quote (the reference
// gets no list back and setup() counts its entries anyway)
bool split_quoted(const std::string &line, std::vector<std::string> &out) {
    out.clear();
    const char *s = line.c_str();
    const int len = (int) line.size();
    int i = 0;
    while (i < len) {
        const char *t = s + i;
        const char *in = t;
        while (*in == ' ') in++;
        int end;
        if (*in != '"' && *in != '\'') {
            int l = (int) strlen(in);
            const char *sep = (const char *) memchr(in, ' ', (size_t) l);
            if (sep && sep > in) l = (int) (sep - in);
            out.emplace_back(in, (size_t) l);
            end = (int) (in - t) + l;
        }
        else {
            // quoted_string_len
            const char quote = *in;
            const char *q = in + 1;
            int ql = 0;
            char qs = quote;
            while (qs != 0) {
                const char c = *q++;
                if (c == '\0') return false;
                if (c == '\\') { if (*q == quote || *q == '\\') q++; }
                else if ((c == '\'' || c == '"') && c == qs) qs = 0;
                ql++;
            }
            ql--;
            const char *p = in + 1;
            std::string tok;
            for (int k = 0; k < ql; k++) {
                if (*p == '\\' && (p[1] == quote || p[1] == '\\')) p++;
                tok.push_back(*p++);
            }
            out.push_back(tok);
            end = (int) (p - t);
        }
        i += end;
        i++;
        if (out.size() >= 3 && i < len) { out.emplace_back(s + i, (size_t) (len - i)); break; }
    }
    return true;
}

struct MItem {
    bool cond;
    int type;
    std::string k, v;           // rule: key / value; condition: a / b
    bool has_b;
    // condition: the accessor's first part (src/flb_record_accessor.c:74-230,767-779)
    int ra;                     // 0 never finds a value, 1 a key (DevKey below)
    DevKey key;
};

// flb_regex_create's verdict; exec: the pattern runs per record and has to be a regular expression the device runs
bool check_rx(const std::string &pat, bool exec, std::string &why, rx::Program *prog_out) {
    const char *ps, *pe;
    unsigned opts;
    rx::split_flb_pattern(pat.c_str(), &ps, &pe, &opts);
    rx::Program prog;
    std::string err;
    if (rx::compile(ps, (size_t) (pe - ps), opts, false, prog, err)) {
        if (prog_out) *prog_out = std::move(prog);
        return true;
    }
    if (prog.nonregular) {
        std::string e2;
        rx::BtProgram *bt = rx::bt_compile(ps, (size_t) (pe - ps), opts, e2);
        if (bt) {
            rx::bt_free(bt);
            if (!exec) return true;
            why = "pattern '" + pat + "' is not a regular expression (" + err + "): a pattern filter_modify runs per record must be one";
            return false;
        }
        err = e2;
    }
    why = "Unable to create regex from '" + pat + "': " + err;
    return false;
}

// the accessor of a condition's `a`: flb_ra_create(a, FLB_FALSE), then get_ra_parser -- the FIRST part decides
bool cond_accessor(const std::string &a, MItem &it, std::string &why) {
    it.ra = 0;
    memset(&it.key, 0, sizeof(it.key));
    const size_t dollar = a.find('$');
    std::string name;
    if (dollar == std::string::npos || dollar > 0) {
        // a string part (src/record_accessor/flb_ra_parser.c:224-249): its text is the key name
        name = dollar == std::string::npos ? a : a.substr(0, dollar);
        if (name.empty()) return true;
        if (name.size() >= (size_t) MAX_KEY) { why = "condition key longer than " + std::to_string(MAX_KEY - 1) + " bytes"; return false; }
        it.ra = 1;
        it.key.is_ra = 1;
        memcpy(it.key.key, name.data(), name.size());
        it.key.key_len = (int) name.size();
        return true;
    }
    if (a.size() == 1) return true;                                     // "$" alone: no part at all
    if (isdigit((unsigned char) a[1])) return true;                     // $0 .. $9: a regex id
    if (a.size() >= 4 && a.compare(1, 3, "TAG") == 0) return true;      // $TAG, $TAG[n]
    size_t end = 1;
    int quotes = 0;
    for (; end < a.size(); end++) {
        const char c = a[end];
        if (c == '\'') quotes++;
        else if (c == '.' && (quotes & 1)) continue;
        else if (c == '.' || c == ' ' || c == ',' || c == '"') break;
    }
    std::string w2;
    if (!parse_ra(a.substr(0, end).c_str(), it.key, w2)) { why = "record accessor '" + a + "': " + w2; return false; }
    it.ra = 1;
    return true;
}

const char *const RULE_NAMES1[] = {"remove", "remove_wildcard", "remove_regex", "move_to_start", "move_to_end"};
const int RULE_TYPES1[] = {MR_REMOVE, MR_REMOVE_WILDCARD, MR_REMOVE_REGEX, MR_MOVE_TO_START, MR_MOVE_TO_END};
// (setup() also knows "add_if_not_present" (:447-452), but the config map (:1589-1655) does not: the filter refuses it before setup() runs)
const char *const RULE_NAMES2[] = {"rename", "hard_rename", "add", "set", "copy", "hard_copy"};
const int RULE_TYPES2[] = {MR_RENAME, MR_HARD_RENAME, MR_ADD, MR_SET, MR_COPY, MR_HARD_COPY};
const char *const COND_NAMES[] = {"key_exists", "key_does_not_exist", "a_key_matches", "no_key_matches", "key_value_equals",
                                  "key_value_does_not_equal", "key_value_matches", "key_value_does_not_match",
                                  "matching_keys_have_matching_values", "matching_keys_do_not_have_matching_values"};

bool cond_a_rx(int t) { return t == MC_A_KEY_MATCHES || t == MC_NO_KEY_MATCHES || t >= MC_MATCHING_KEYS_HAVE_MATCHING_VALUES; }
bool cond_b_rx(int t) { return t == MC_KEY_VALUE_MATCHES || t == MC_KEY_VALUE_DOES_NOT_MATCH || t >= MC_MATCHING_KEYS_HAVE_MATCHING_VALUES; }

// setup() (:141-519) over the properties in configuration order
bool parse_program(int nprops, const char *const *names, const char *const *values, std::vector<MItem> &items, std::string &why) {
    items.clear();
    int nrules = 0, nconds = 0;
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        std::vector<std::string> tok;
        if (!split_quoted(val, tok)) { why = "unterminated quote in " + name + " " + val; return false; }
        if (tok.empty() || tok.size() > 3) { why = "Invalid config for " + name; return false; }
        MItem it;
        it.has_b = false; it.ra = 0;
        memset(&it.key, 0, sizeof(it.key));
        if (!strcasecmp(name.c_str(), "condition")) {
            it.cond = true;
            it.type = -1;
            for (int t = 0; t < 10; t++) if (!strcasecmp(tok[0].c_str(), COND_NAMES[t])) it.type = t;
            if (it.type < 0) { why = "Invalid config for " + name + " : " + val; return false; }
            // (a Condition of one token makes the reference read past its list, :280-285)
            if (tok.size() < 2) { why = "Invalid config for " + name + " : " + val + " (no key)"; return false; }
            it.k = tok[1];
            if (tok.size() == 3) { it.v = tok[2]; it.has_b = true; }
            if (cond_a_rx(it.type)) {
                if (it.k.empty()) { why = "Unable to create regex for condition " + name + " " + val; return false; }
                if (!check_rx(it.k, true, why, nullptr)) return false;
            }
            if (cond_b_rx(it.type)) {
                if (it.v.empty()) { why = "Unable to create regex for condition " + name + " " + val; return false; }
                if (!check_rx(it.v, true, why, nullptr)) return false;
            }
            if (!cond_a_rx(it.type) && !cond_accessor(it.k, it, why)) return false;
            if (++nconds > MOD_MAX_CONDS) { why = "more than " + std::to_string(MOD_MAX_CONDS) + " conditions"; return false; }
        }
        else {
            it.cond = false;
            it.type = -1;
            it.k = tok.front(); it.v = tok.back();
            bool known = false;
            for (int t = 0; t < 5; t++) if (!strcasecmp(name.c_str(), RULE_NAMES1[t])) { known = true; if (tok.size() == 1) it.type = RULE_TYPES1[t]; }
            for (int t = 0; t < 6; t++) if (!strcasecmp(name.c_str(), RULE_NAMES2[t])) { known = true; if (tok.size() == 2) it.type = RULE_TYPES2[t]; }
            // three tokens: the rule type stays at calloc's 0, RENAME (modify.h:28-29), of the first token to the last
            if (known && tok.size() == 3) it.type = MR_RENAME;
            if (it.type < 0) { why = "Invalid operation " + name + " : " + val + " in configuration"; return false; }
            if (it.type == MR_REMOVE_REGEX && it.k.empty()) { why = "Unable to create regex for rule " + name + " " + val; return false; }
            // every rule's key and value go through flb_regex_create (:478-507); only Remove_regex's key runs
            if (!check_rx(it.k, it.type == MR_REMOVE_REGEX, why, nullptr)) return false;
            if (!check_rx(it.v, false, why, nullptr)) return false;
            // Hard_copy k k packs a map header one larger than its entries (:1142-1161)
            if (it.type == MR_HARD_COPY && it.k == it.v) { why = "Hard_copy of a key onto itself (" + it.k + ") is refused"; return false; }
            if (++nrules > MOD_MAX_RULES) { why = "more than " + std::to_string(MOD_MAX_RULES) + " rules"; return false; }
        }
        items.push_back(it);
    }
    return true;
}

std::string describe(const std::vector<MItem> &items) {
    std::string d;
    for (const MItem &it : items) {
        if (!d.empty()) d += ";";
        if (!it.cond) { d += "R" + std::to_string(it.type) + "," + hexs(it.k) + "," + hexs(it.v); continue; }
        d += "C" + std::to_string(it.type) + "," + hexs(it.k) + "," + (it.has_b ? hexs(it.v) : std::string("-"));
        if (cond_a_rx(it.type)) continue;
        if (!it.ra) { d += ",N"; continue; }
        d += ",K" + hexs(std::string(it.key.key, (size_t) it.key.key_len));
        for (int s = 0; s < it.key.nsub; s++) {
            if (it.key.sub_is_index[s]) d += "/i" + std::to_string(it.key.sub_index[s]);
            else d += "/s" + hexs(std::string(it.key.sub_str + it.key.sub_off[s], (size_t) it.key.sub_len[s]));
        }
    }
    return d;
}

bool front(int nprops, const char *const *names, const char *const *values, std::vector<MItem> &items) {
    return parse_front("modify", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, items, why); });
}

struct ModState : FilterState {
    struct Words { unsigned long long first_bad, counts[5], arena_top; };
    std::vector<ModRule> rules;
    std::vector<ModCond> conds;
    std::vector<DevKey> keys;
    std::vector<GrepRule> rx;
    std::string str;
    uint32_t true_off = 0, false_off = 0;
    int grow = 0;
    ScopedDevBuf d_rules, d_conds, d_keys, d_rx, d_str, d_arena;
    CallWords<Words> words;
    uint64_t arena_cap = 0;
    uint64_t overread = 0;      // records whose prefix test ran past the record (counted difference, DESIGN)
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

}  // namespace

extern "C" int flbgpu_modify_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    std::vector<MItem> items;
    if (!front(nprops, names, values, items)) return -1;
    put_desc(desc, cap, describe(items));
    return 0;
}

static bool add_rx(ModState *m, flbgpu_filter *f, const std::string &pat, int *idx) {
    std::string why;
    rx::Program prog;
    if (!check_rx(pat, true, why, &prog)) { set_err("filter_modify: %s", why.c_str()); return false; }
    GrepRule r;
    memset(&r, 0, sizeof(r));
    if (!upload_rule(prog, r, f->rule_blobs)) return false;
    *idx = (int) m->rx.size();
    m->rx.push_back(r);
    return true;
}

extern "C" flbgpu_filter *flbgpu_filter_modify_create(int nprops, const char *const *names, const char *const *values) {
    std::vector<MItem> items;
    if (!front(nprops, names, values, items)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_MODIFY;
    auto *m = new ModState();
    f->state = m;
    auto add_str = [&](const std::string &s) { const uint32_t o = (uint32_t) m->str.size(); m->str += s; return o; };
    m->true_off = add_str("true");
    m->false_off = add_str("false");
    for (const MItem &it : items) {
        if (it.cond) {
            ModCond c;
            memset(&c, 0, sizeof(c));
            c.type = it.type; c.key = -1; c.rx_a = -1; c.rx_b = -1;
            if (it.has_b) { c.b_off = add_str(it.v); c.b_len = (uint32_t) it.v.size(); }
            if (cond_a_rx(it.type) && !add_rx(m, f, it.k, &c.rx_a)) { delete f; return nullptr; }
            if (cond_b_rx(it.type) && !add_rx(m, f, it.v, &c.rx_b)) { delete f; return nullptr; }
            if (!cond_a_rx(it.type) && it.ra) { c.key = (int) m->keys.size(); m->keys.push_back(it.key); }
            m->conds.push_back(c);
        }
        else {
            ModRule r;
            memset(&r, 0, sizeof(r));
            r.type = it.type; r.rx = -1;
            r.k_off = add_str(it.k); r.k_len = (uint32_t) it.k.size();
            r.v_off = add_str(it.v); r.v_len = (uint32_t) it.v.size();
            if (it.type == MR_REMOVE_REGEX && !add_rx(m, f, it.k, &r.rx)) { delete f; return nullptr; }
            if (it.type == MR_ADD || it.type == MR_SET || it.type == MR_COPY || it.type == MR_HARD_COPY) m->grow++;
            m->rules.push_back(r);
        }
    }
    if (!filter_common_init(f) || !upload(m->d_rules, m->rules) || !upload(m->d_conds, m->conds) || !upload(m->d_keys, m->keys) ||
        !upload(m->d_rx, m->rx) || !upload(m->d_str, m->str.data(), m->str.size())) {
        delete f;
        return nullptr;
    }
    return f;
}

extern "C" uint64_t flbgpu_modify_overread(flbgpu_filter *f) {
    auto *m = state_of<ModState>(f, F_MODIFY);
    return m ? m->overread : 0;
}

constexpr uint64_t MOD_ARENA_INIT = 1u << 16;      // entries (512 KB): the arena a filter keeps between calls

// cb_modify_filter (:1486-1578) on a device chunk: MODIFIED only when a record was rebuilt AND the decoder reached the end of the chunk
bool ModState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) {
    const uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0) return true;
    if (!words.ensure() || !ensure_row_columns(f, n)) return false;
    if (arena_cap == 0) {
        arena_cap = MOD_ARENA_INIT;
        if (!d_arena.ensure(arena_cap * sizeof(uint64_t))) return false;
    }
    // an arena grown for this call's wide maps is handed back when the call ends (every return path)
    struct ArenaTrim {
        ModState *m;
        ~ArenaTrim() { if (m->arena_cap > MOD_ARENA_INIT) { m->d_arena.release(); m->arena_cap = 0; } }
    } trim{this};
    Words *dw = words.dev();
    Words &hw = words.host();
    ModArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.rules = d_rules.as<ModRule>(); a.nrules = (int) rules.size();
    a.conds = d_conds.as<ModCond>(); a.nconds = (int) conds.size();
    a.keys = d_keys.as<DevKey>(); a.rx = d_rx.as<GrepRule>(); a.str = d_str.as<uint8_t>();
    a.true_off = true_off; a.false_off = false_off; a.grow = grow;
    a.len = f->d_len.as<uint32_t>();
    a.first_bad = &dw->first_bad; a.counts = dw->counts; a.arena_top = &dw->arena_top;
    // first_bad: what the words start from -- nothing refused yet, or, for the pass in front of a decoder error, that record
    auto size_pass = [&](const char *name, unsigned long long first_bad) {
        return words.pass(f, st, name, [&](Words &w) { memset(&w, 0, sizeof(w)); w.first_bad = first_bad; }, [&] { launch_modify(a, false, st); });
    };
    for (int attempt = 0;; attempt++) {
        a.arena = d_arena.as<uint64_t>(); a.arena_cap = arena_cap;
        if (!size_pass("k_modify(size)", ~0ull)) return false;
        if (hw.counts[4] >> 32) { set_err("filter_modify: a record's output is larger than 4 GB"); return false; }
        if ((hw.counts[4] & 0xFFFFFFFFull) == 0) break;
        // rows with more entries than a lane's LDS list holds: their lists did not all fit in the arena -- grow it, size again
        if (attempt > 0) { set_err("filter_modify: the entry arena did not grow"); return false; }
        d_arena.release();
        arena_cap = hw.counts[3] + hw.counts[3] / 4 + 1024;
        if (!d_arena.ensure(arena_cap * sizeof(uint64_t))) return false;
    }
    if (hw.first_bad != ~0ull && hw.first_bad > 0) {
        // the reference's decoder loop stops at the first bad record: the records it decoded, and its prefix tests, are the ones in
        // front of it -- the size pass again over those rows only (a call that ends in NOTOUCH anyway)
        const unsigned long long fb = hw.first_bad;
        a.n = fb;
        if (!size_pass("k_modify(size, in front of a decoder error)", fb)) return false;
        hw.first_bad = fb;
    }
    else if (hw.first_bad == 0) hw.counts[0] = hw.counts[2] = 0;
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[0];
    overread += hw.counts[2];
    // a decoder error anywhere (or a tail that is not a clean end) and the reference answers NOTOUCH (:1549-1571); so does a call
    // that rebuilt nothing
    if (hw.first_bad != ~0ull || garbage || hw.counts[1] == 0) return true;
    if (!scan_lengths(f, st, a.len, n, &words.total())) return false;
    HIPOK(hipMemsetAsync(&dw->arena_top, 0, sizeof(dw->arena_top), st));
    a.out_off = f->d_off.as<uint64_t>(); a.out = f->d_out.as<uint8_t>();
    { ProfScope ps(f, st, "k_modify(emit)"); launch_modify(a, true, st); }
    HIPOK(hipStreamSynchronize(st));
    set_out(f, out, n, words.total());
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
