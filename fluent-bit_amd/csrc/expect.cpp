// expect.cpp -- filter_expect (plugins/filter_expect/expect.c): the configuration as the config map (:580-632) and context_create
// (:146-230) read it, the rule table for LDS, one cb_expect_filter call on a device chunk (:398-564), and the last call's failures
// with the messages rule_apply (:275-396) logs for them.  The per-record work is expect_kernels.inc.
#include "filter_host.hpp"
#include "expect.hpp"

using namespace flbgpu;

namespace {

struct ERule {
    int kind = EX_KEY_EXISTS;
    std::string value;                   // the property's value as it was configured: the messages quote it (rule->value)
    bool inert = true;                   // the accessor has no key part: nothing is ever found
    DevKey key;
    std::string expect;                  // key_val_eq
};

struct EProgram {
    int action = EX_WARN;
    std::string result_key = "matched";
    std::vector<ERule> rules;
};

const char *const ACTIONS[] = {"warn", "exit", "result_key"};
const char *const KINDS[] = {"key_exists", "key_not_exists", "key_val_is_null", "key_val_is_not_null", "key_val_eq", "action"};

// flb_slist_split_string(list, s, ' ', 1) (src/flb_slist.c:223-313): the first run of bytes that are no spaces, then -- behind the
// spaces that follow it -- the rest of the line as it is
void split_string(const std::string &s, std::vector<std::string> &out) {
    out.clear();
    size_t i = 0;
    while (i < s.size() && s[i] == ' ') i++;
    if (i == s.size()) return;
    size_t j = s.find(' ', i);
    if (j == std::string::npos) { out.push_back(s.substr(i)); return; }
    out.push_back(s.substr(i, j - i));
    while (j < s.size() && s[j] == ' ') j++;
    if (j < s.size()) out.push_back(s.substr(j));
}

// flb_ra_create(text, FLB_TRUE), then get_ra_parser: the first part decides (src/flb_record_accessor.c:767-779)
bool accessor(const std::string &text, ERule &r, std::string &why) {
    std::vector<RaPart> parts;
    std::string w;
    const int rc = ra_split(text, parts, w);
    if (!parts.empty() && parts[0].kind == RA_STR && parts[0].str.size() >= (size_t) MAX_KEY) {
        why = "'" + text + "': key longer than " + std::to_string(MAX_KEY - 1) + " bytes";
        return false;
    }
    if (rc == RA_SPLIT_SKIP) { why = "error processing accessor key '" + text + "'"; return false; }
    if (rc == RA_SPLIT_REFUSE) { why = "'" + text + "': " + w; return false; }
    memset(&r.key, 0, sizeof(r.key));
    r.inert = parts.empty() || (parts[0].kind != RA_STR && parts[0].kind != RA_KEY);
    if (r.inert) return true;
    if (parts[0].kind == RA_KEY) r.key = parts[0].key;
    else {
        r.key.is_ra = 1;
        memcpy(r.key.key, parts[0].str.data(), parts[0].str.size());
        r.key.key_len = (int) parts[0].str.size();
    }
    return true;
}

int kind_of(const char *n) {
    for (int k = 0; k < 5; k++) if (!strcasecmp(n, KINDS[k])) return k;
    return -1;
}

// the config map (:580-632) and context_create (:146-230) over the properties in configuration order
bool parse_program(int nprops, const char *const *names, const char *const *values, EProgram &pg, std::string &why) {
    int seen_action = 0, seen_key = 0;
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        const char *n = name.c_str();
        // (the engine translates ${VAR} in every value when the property is set: src/flb_filter.c flb_filter_set_property)
        if (val.find("${") != std::string::npos) { why = name + " '" + val + "': environment variables are not translated"; return false; }
        // a property without FLB_CONFIG_MAP_MULT that is set more than once fails the check of the properties (src/flb_config_map.c:551-560)
        if (!strcasecmp(n, "action")) {
            if (++seen_action > 1) { why = "configuration property '" + name + "' is set more than once"; return false; }
            int a = -1;
            for (int k = 0; k < 3; k++) if (!strcasecmp(val.c_str(), ACTIONS[k])) a = k;
            if (a < 0) { why = "unexpected 'action' value '" + val + "'"; return false; }
            pg.action = a;
        }
        else if (!strcasecmp(n, "result_key")) {
            if (++seen_key > 1) { why = "configuration property '" + name + "' is set more than once"; return false; }
            pg.result_key = val;
        }
        else if (kind_of(n) < 0) { why = "unknown configuration rule '" + name + "'"; return false; }
    }
    if (pg.result_key.size() > EX_MAX_RESULT_KEY) { why = "result_key longer than " + std::to_string(EX_MAX_RESULT_KEY) + " bytes"; return false; }
    // the rules: every property but result_key, `action` included -- its rule has no type, passes always and takes a number (:194-226)
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        if (!strcasecmp(name.c_str(), "result_key")) continue;
        ERule r;
        r.value = val;
        memset(&r.key, 0, sizeof(r.key));
        if (!strcasecmp(name.c_str(), "action")) r.kind = EX_ACTION;       // (its value is one of three words: an accessor without a key)
        else {
            r.kind = kind_of(name.c_str());
            std::string acc = val;
            if (r.kind == EX_KEY_VAL_EQ) {
                std::vector<std::string> tok;
                split_string(val, tok);
                // the reference takes the first and the last entry of the list, and of an empty list too (:91-92)
                if (tok.empty()) { why = "key_val_eq needs 'KEY VALUE': '" + val + "'"; return false; }
                acc = tok.front();
                r.expect = tok.back();
            }
            if (!accessor(acc, r, why)) { why = name + " " + why; return false; }
        }
        pg.rules.push_back(r);
        if ((int) pg.rules.size() > EX_MAX_RULES) { why = "more than " + std::to_string(EX_MAX_RULES) + " rules"; return false; }
    }
    return true;
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
    else { o.push_back((char) 0xda); o.push_back((char) (n >> 8)); o.push_back((char) n); }
    return o + s;
}

// the LDS table of expect.hpp
void build_table(const EProgram &pg, std::vector<uint32_t> &table) {
    table.assign(EX_HDR_WORDS + EX_RULE_WORDS * pg.rules.size(), 0);
    const std::string rk = packed_str(pg.result_key);
    table[0] = (uint32_t) pg.rules.size();
    table[1] = (uint32_t) pg.action;
    table[2] = (uint32_t) rk.size();
    table[3] = (uint32_t) (table.size() * 4);
    put_bytes(table, rk.data(), rk.size());
    for (size_t i = 0; i < pg.rules.size(); i++) {
        const ERule &r = pg.rules[i];
        uint32_t w[EX_RULE_WORDS] = {(uint32_t) r.kind, EX_ACC_INERT, 0, 0, 0, 0, 0, 0};
        if (!r.inert) {
            w[1] = (uint32_t) r.key.key_len | ((uint32_t) r.key.nsub << 16);
            w[2] = (uint32_t) (table.size() * 4);
            put_bytes(table, r.key.key, (size_t) r.key.key_len);
            const size_t sub = table.size();
            w[3] = (uint32_t) (sub * 4);
            table.resize(sub + 2 * (size_t) r.key.nsub, 0);
            for (int s = 0; s < r.key.nsub; s++) {
                if (r.key.sub_is_index[s]) { table[sub + 2 * s] = (uint32_t) r.key.sub_index[s] | TC_SUB_INDEX; continue; }
                table[sub + 2 * s] = (uint32_t) r.key.sub_len[s];
                table[sub + 2 * s + 1] = (uint32_t) (table.size() * 4);
                put_bytes(table, r.key.sub_str + r.key.sub_off[s], (size_t) r.key.sub_len[s]);
            }
        }
        if (r.kind == EX_KEY_VAL_EQ) {
            w[4] = (uint32_t) r.expect.size();
            w[5] = (uint32_t) (table.size() * 4);
            put_bytes(table, r.expect.data(), r.expect.size());
        }
        memcpy(&table[EX_HDR_WORDS + EX_RULE_WORDS * i], w, sizeof(w));
    }
}

std::string describe(const EProgram &pg) {
    std::string d = std::string("action=") + ACTIONS[pg.action] + ";result_key=" + hexs(pg.result_key);
    for (size_t i = 0; i < pg.rules.size(); i++) {
        const ERule &r = pg.rules[i];
        d += ";#" + std::to_string(i) + ":" + KINDS[r.kind] + ":";
        if (r.inert) d += "-";
        else {
            d += "K" + hexs(std::string(r.key.key, (size_t) r.key.key_len));
            for (int s = 0; s < r.key.nsub; s++) {
                if (r.key.sub_is_index[s]) d += "[" + std::to_string(r.key.sub_index[s]) + "]";
                else d += "." + hexs(std::string(r.key.sub_str + r.key.sub_off[s], (size_t) r.key.sub_len[s]));
            }
        }
        if (r.kind == EX_KEY_VAL_EQ) d += ":E" + hexs(r.expect);
    }
    return d;
}

bool checked_program(int nprops, const char *const *names, const char *const *values, EProgram &pg, std::vector<uint32_t> &table) {
    if (!parse_front("expect", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, pg, why); })) return false;
    build_table(pg, table);
    if (table.size() * 4 > TC_MAX_TABLE_BYTES) { set_err("filter_expect: rule table larger than %u bytes", TC_MAX_TABLE_BYTES); return false; }
    return true;
}

struct ExpectState : FilterState {
    struct Words { unsigned long long firsts[2], counts[5]; };
    EProgram pg;
    uint32_t table_bytes = 0;
    uint64_t checked = 0, failed = 0, exits = 0, mismatch = 0;            // since the filter was created (flbgpu_expect_counters)
    ScopedDevBuf d_table, d_verdict, d_voff, d_vlen, d_fail, d_fidx, d_ftbl;
    CallWords<Words> words;
    // the last call's failures
    uint64_t last_n = 0;                  // on the device
    bool on_host = true;
    std::vector<ExFailure> h_tbl;
    std::vector<uint8_t> h_input;
    const uint8_t *input = nullptr;       // host-level call: the bytes the offsets index
    uint64_t input_bytes = 0;
    const uint8_t *dev_data = nullptr;    // the chunk the offsets index, on the device
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
    bool table_to_host();
};

bool ExpectState::table_to_host() {
    if (on_host) return true;
    h_tbl.resize(last_n);
    if (last_n && hipMemcpy(h_tbl.data(), d_ftbl.p, last_n * sizeof(ExFailure), hipMemcpyDeviceToHost) != hipSuccess) { set_err("device read failed"); return false; }
    on_host = true;
    return true;
}

}  // namespace

extern "C" int flbgpu_expect_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    EProgram pg;
    std::vector<uint32_t> table;
    if (!checked_program(nprops, names, values, pg, table)) return -1;
    put_desc(desc, cap, describe(pg));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_expect_create(int nprops, const char *const *names, const char *const *values) {
    EProgram pg;
    std::vector<uint32_t> table;
    if (!checked_program(nprops, names, values, pg, table)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_EXPECT;
    auto *m = new ExpectState();
    f->state = m;
    m->pg = pg;
    m->table_bytes = (uint32_t) (table.size() * 4);
    if (!filter_common_init(f) || !upload(m->d_table, table)) {
        set_err("filter_expect: the rule table could not be placed on the device");
        delete f;
        return nullptr;
    }
    return f;
}

extern "C" void flbgpu_expect_counters(flbgpu_filter *f, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (auto *m = state_of<ExpectState>(f, F_EXPECT)) { out[0] = m->checked; out[1] = m->failed; out[2] = m->exits; out[3] = m->mismatch; }
}

static_assert(sizeof(ExFailure) == sizeof(flbgpu_expect_failure), "the failure table's entry is the C ABI's");

extern "C" int flbgpu_expect_failures(flbgpu_filter *f, flbgpu_expect_failures_t *out) {
    if (!out) return -1;
    memset(out, 0, sizeof(*out));
    ExpectState *m = state_of<ExpectState>(f, F_EXPECT);
    if (!m) { set_err("filter_expect: not an expect filter"); return -1; }
    if (!m->table_to_host()) return -1;
    out->count = m->h_tbl.size();
    out->recs = (const flbgpu_expect_failure *) m->h_tbl.data();
    out->input = m->input;
    out->input_bytes = m->input_bytes;
    return 0;
}

extern "C" int flbgpu_expect_failures_dev(flbgpu_filter *f, flbgpu_expect_failures_t *out) {
    if (!out) return -1;
    memset(out, 0, sizeof(*out));
    ExpectState *m = state_of<ExpectState>(f, F_EXPECT);
    if (!m) { set_err("filter_expect: not an expect filter"); return -1; }
    out->count = m->last_n;
    out->recs = m->last_n ? (const flbgpu_expect_failure *) m->d_ftbl.p : nullptr;
    return 0;
}

// the message rule_apply hands flb_plg_error (:295-387), up to and including "Record content:\n"; val: the STR value a key_val_eq met
static bool failure_message(const EProgram &pg, uint64_t rule, uint32_t kind, uint32_t vtype, const std::string &val, std::string &t) {
    if (rule >= pg.rules.size() || pg.rules[rule].kind == EX_ACTION) { set_err("filter_expect: no rule #%llu that can fail", (unsigned long long) rule); return false; }
    const ERule &r = pg.rules[rule];
    static const char *const types[] = {"", "boolean", "integer", "float / double", "string", "null", "UNKNOWN"};
    t = "exception on rule #" + std::to_string(rule) + " ";
    if (r.kind == EX_KEY_EXISTS) t += "'key_exists', key '" + r.value + "' not found.";
    else if (r.kind == EX_KEY_NOT_EXISTS) t += "'key_not_exists', key '" + r.value + "' exists.";
    else if (kind == EXF_NOT_FOUND)                                // key_val_eq says 'key_val_is_null' here too (:366-373)
        t += std::string("'") + (r.kind == EX_KEY_VAL_NOT_NULL ? KINDS[EX_KEY_VAL_NOT_NULL] : KINDS[EX_KEY_VAL_NULL]) + "', key '" + r.value + "' not found.";
    else if (kind == EXF_WRONG_TYPE)
        t += std::string("'") + KINDS[r.kind] + "', key '" + r.value + "' contains a value type '" + types[vtype < 7 ? vtype : 6] + "'.";
    else                                                           // the value is printed with %s: it ends at its first NUL
        t += "'key_val_eq', key value '" + std::string(val.c_str()) + "' is different than expected: '" + r.expect + "'.";
    t += " Record content:\n";
    return true;
}

extern "C" int flbgpu_expect_text_check(int nprops, const char *const *names, const char *const *values, uint64_t rule, uint32_t kind, uint32_t vtype,
                                        const void *val, size_t val_len, char *buf, size_t cap) {
    EProgram pg;
    std::vector<uint32_t> table;
    std::string t;
    if (!checked_program(nprops, names, values, pg, table)) return -1;
    if (!failure_message(pg, rule, kind, vtype, std::string(val ? (const char *) val : "", val ? val_len : 0), t)) return -1;
    put_desc(buf, cap, t);
    return (int) t.size();
}

extern "C" int flbgpu_expect_failure_text(flbgpu_filter *f, uint64_t i, char *buf, size_t cap) {
    ExpectState *m = state_of<ExpectState>(f, F_EXPECT);
    if (!m) { set_err("filter_expect: not an expect filter"); return -1; }
    if (!m->table_to_host()) return -1;
    if (i >= m->h_tbl.size()) { set_err("filter_expect: no failure %llu", (unsigned long long) i); return -1; }
    const ExFailure &e = m->h_tbl[i];
    std::string v, t;
    if (e.kind == EXF_DIFFERENT && e.val_len) {
        v.assign(e.val_len, '\0');
        if (m->input && e.val_off + e.val_len <= m->input_bytes) memcpy(&v[0], m->input + e.val_off, e.val_len);
        else if (!m->dev_data || hipMemcpy(&v[0], m->dev_data + e.val_off, e.val_len, hipMemcpyDeviceToHost) != hipSuccess) { set_err("device read failed"); return -1; }
    }
    if (!failure_message(m->pg, e.rule, e.kind, e.vtype, v, t)) return -1;
    put_desc(buf, cap, t);
    return (int) t.size();
}

// cb_expect_filter (:398-564) on a device chunk.  warn and exit only look: the call answers NOTOUCH whatever the rules say.  result_key
// rebuilds every record and answers MODIFIED when the decoder's loop ended on a clean end of data (:535-538); a decoder error or
// undecodable bytes behind the rows (`garbage`) leave NOTOUCH, the rules having run on the records in front of it all the same.
bool ExpectState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) {
    uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    last_n = 0; on_host = true; h_tbl.clear(); input = nullptr; input_bytes = 0; dev_data = (const uint8_t *) in->data;
    if (n == 0) return true;
    if (!words.ensure() || !ensure_row_columns(f, n) || !d_verdict.ensure(n * 4) || !d_voff.ensure(n * 4) || !d_vlen.ensure(n * 4) ||
        !d_fail.ensure(n * 4) || !d_fidx.ensure((n + 1) * 8))
        return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    uint64_t &total = words.total();
    ExpectArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = table_bytes;
    a.verdict = d_verdict.as<uint32_t>(); a.val_off = d_voff.as<uint32_t>(); a.val_len = d_vlen.as<uint32_t>(); a.fail = d_fail.as<uint32_t>();
    a.len = f->d_len.as<uint32_t>();
    a.firsts = dw->firsts; a.counts = dw->counts;
    int pass = pg.action == EX_RESULT_KEY && !garbage ? EX_SIZE : EX_CHECK;
    auto look = [&](const char *name) {
        return words.pass(f, st, name, [](Words &w) { memset(w.firsts, 0xff, sizeof(w.firsts)); memset(w.counts, 0, sizeof(w.counts)); },
                          [&] { launch_expect(a, pass, st); });
    };
    if (!look(pass == EX_SIZE ? "k_expect(size)" : "k_expect(check)")) return false;
    if (hw.firsts[0] != ~0ull) {
        // the loop ends at the first record the decoder refuses: the call is the rows in front of it, and it hands nothing on
        pass = EX_CHECK;
        a.n = n = hw.firsts[0];
        if (n == 0) return true;
        if (!look("k_expect(check, in front of a decoder error)")) return false;
    }
    if (pg.action == EX_EXIT && hw.firsts[1] != ~0ull) {
        // the loop ends at the first failure (:445-448): what stands behind it is not checked
        a.n = n = hw.firsts[1] + 1;
        if (!look("k_expect(check, up to the first failure)")) return false;
        exits++;
    }
    if (hw.counts[3]) { set_err("filter_expect: a record is larger than 4 GB"); return false; }
    checked += hw.counts[0]; failed += hw.counts[1];
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[0];
    const uint64_t nf = hw.counts[1];
    if (nf) {
        // the failure table in record order: a scan over the fail flags places every entry
        if (!d_ftbl.ensure(nf * sizeof(ExFailure) + 16)) return false;
        { ProfScope ps(f, st, "k_scan"); launch_scan(a.fail, n, f->d_scan_tmp.as<uint64_t>(), d_fidx.as<uint64_t>(), st, nullptr); }
        a.fail_idx = d_fidx.as<uint64_t>(); a.fail_tbl = d_ftbl.as<ExFailure>(); a.fail_cap = nf;
        { ProfScope ps(f, st, "k_expect_table"); launch_expect_table(a, st); }
        HIPOK(hipStreamSynchronize(st));
        last_n = nf; on_host = false;
        if (f->rtag_host_call) {
            // a host-level call: the offsets index the caller's bytes, or -- behind another filter of a chain -- a copy of this filter's input
            if (!table_to_host()) return false;
            if (in->data == f->rtag_dev_base && f->rtag_host_base) input = f->rtag_host_base;
            else {
                h_input.resize(in->bytes);
                if (in->bytes) HIPOK(hipMemcpy(h_input.data(), in->data, in->bytes, hipMemcpyDeviceToHost));
                input = h_input.data();
            }
            input_bytes = in->bytes;
        }
    }
    if (pass != EX_SIZE) return true;
    if (!scan_lengths(f, st, a.len, n, &total)) return false;
    if (total == 0) {                                                    // group markers no encoder took, records it refused: an empty buffer
        memset(out, 0, sizeof(*out));
        f->last_out = 0;
        *ret = FLBGPU_FILTER_MODIFIED;
        return true;
    }
    a.out_off = f->d_off.as<uint64_t>(); a.out = f->d_out.as<uint8_t>();
    { ProfScope ps(f, st, "k_expect(emit)"); launch_expect(a, EX_EMIT, st); }
    HIPOK(hipMemcpyAsync(&hw.counts[4], &dw->counts[4], sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    mismatch += hw.counts[4];
    if (hw.counts[4]) { set_err("filter_expect: %llu rows were emitted with another length than they were sized", hw.counts[4]); return false; }
    set_out(f, out, n, total);
    // (records emitted: the rows that went out without the group markers among them)
    f->last_out = hw.counts[2];
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
