// typeconv.cpp -- filter_type_converter (plugins/filter_type_converter/type_converter.c): the configuration as configure() reads it
// (:108-140, config_rule :57-106, behind the config map of :366-388), the device program behind it, and one
// cb_type_converter_filter call on a device chunk (:182-353).  The per-record work is typeconv_kernels.inc.
#include "filter_host.hpp"
#include "typeconv.hpp"

using namespace flbgpu;

namespace {

struct TRule {
    int src = 0, to = 0;
    bool inert = false;             // the accessor has no key part (get_ra_parser answers NULL): the key is never found
    DevKey key;
    std::string from, to_key;
};
struct TProgram { std::vector<TRule> rules; };

// flb_typecast_str_to_type_t (src/flb_typecast.c:27-49): strncasecmp(word, name, strlen(word)) in this order -- the word is a
// prefix of the name, the empty word of the first one
int type_of_word(const std::string &w) {
    static const char *const names[] = {"int", "uint", "float", "hex", "string", "bool"};
    for (int i = 0; i < 6; i++)
        if (w.size() <= strlen(names[i]) && !strncasecmp(w.c_str(), names[i], w.size())) return i;
    return -1;
}

enum { ACC_KEY = 0, ACC_INERT = 1, ACC_SKIP = 2, ACC_REFUSE = 3 };

// get_ra_parser (src/flb_record_accessor.c:767-779) over the parts ra_split cuts: the FIRST part decides, and only a part with a key
// finds anything -- a `$key...` part, or the plain text in front of the first '$', which the accessor keeps as a key of that name.
// ACC_SKIP: a `$key...` part the accessor's grammar refuses -- flb_ra_create answers NULL.
int accessor(const std::string &a, DevKey &key, std::string &why) {
    std::vector<RaPart> parts;
    const int rc = ra_split(a, parts, why);
    if (!parts.empty() && parts[0].kind == RA_STR && parts[0].str.size() >= (size_t) MAX_KEY) {
        why = "from_key '" + a + "': key longer than " + std::to_string(MAX_KEY - 1) + " bytes";
        return ACC_REFUSE;
    }
    if (rc == RA_SPLIT_SKIP) return ACC_SKIP;
    if (rc == RA_SPLIT_REFUSE) { why = "from_key '" + a + "': " + why; return ACC_REFUSE; }
    if (parts.empty() || (parts[0].kind != RA_STR && parts[0].kind != RA_KEY)) return ACC_INERT;
    if (parts[0].kind == RA_KEY) { key = parts[0].key; return ACC_KEY; }
    memset(&key, 0, sizeof(key));
    key.is_ra = 1;
    memcpy(key.key, parts[0].str.data(), parts[0].str.size());
    key.key_len = (int) parts[0].str.size();
    return ACC_KEY;
}

size_t pad4(size_t n) { return (n + 3) & ~(size_t) 3; }

std::string packed_str(const std::string &s) {
    std::string o;
    const size_t n = s.size();
    if (n < 32) o.push_back((char) (0xa0 | n));
    else if (n < 256) { o.push_back((char) 0xd9); o.push_back((char) n); }
    else if (n < 65536) { o.push_back((char) 0xda); o.push_back((char) (n >> 8)); o.push_back((char) n); }
    else { o.push_back((char) 0xdb); for (int i = 3; i >= 0; i--) o.push_back((char) (n >> (8 * i))); }
    return o + s;
}

void put_bytes(std::vector<uint32_t> &table, const char *s, size_t n) {
    for (size_t j = 0; j < n; j += 4) {
        uint32_t w = 0;
        for (size_t b = 0; b < 4 && j + b < n; b++) w |= (uint32_t) (unsigned char) s[j + b] << (8 * b);
        table.push_back(w);
    }
}

// the table of typeconv.hpp
void build_table(const TProgram &pg, std::vector<uint32_t> &table) {
    table.assign(TC_RULE_WORDS * pg.rules.size(), 0);
    for (size_t i = 0; i < pg.rules.size(); i++) {
        const TRule &r = pg.rules[i];
        const size_t sub = table.size();
        table.resize(sub + 2 * (size_t) r.key.nsub, 0);
        for (int s = 0; s < r.key.nsub; s++) {
            if (r.key.sub_is_index[s]) { table[sub + 2 * s] = (uint32_t) r.key.sub_index[s] | TC_SUB_INDEX; continue; }
            table[sub + 2 * s] = (uint32_t) r.key.sub_len[s];
            table[sub + 2 * s + 1] = (uint32_t) (table.size() * 4);
            put_bytes(table, r.key.sub_str + r.key.sub_off[s], (size_t) r.key.sub_len[s]);
        }
        uint32_t *w = &table[TC_RULE_WORDS * i];
        w[0] = (uint32_t) r.src | ((uint32_t) r.to << 8) | ((uint32_t) r.key.nsub << 16) | (r.inert ? TC_INERT : 0u);
        w[1] = (uint32_t) r.key.key_len;
        w[2] = (uint32_t) (table.size() * 4);
        w[5] = (uint32_t) (sub * 4);
        put_bytes(table, r.key.key, (size_t) r.key.key_len);
        const std::string tk = packed_str(r.to_key);
        w = &table[TC_RULE_WORDS * i];
        w[3] = (uint32_t) tk.size();
        w[4] = (uint32_t) (table.size() * 4);
        put_bytes(table, tk.data(), tk.size());
    }
}

// the config map (:366-388) and configure() (:108-140) over the properties in configuration order
bool parse_program(int nprops, const char *const *names, const char *const *values, TProgram &pg, std::string &why) {
    static const char *const props[] = {"str_key", "int_key", "uint_key", "float_key"};      // configure()'s order
    static const int src_of[] = {TC_SRC_STR, TC_SRC_INT, TC_SRC_UINT, TC_SRC_FLOAT};
    std::vector<std::vector<std::string>> group[4];
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        int g = -1;
        for (int k = 0; k < 4; k++) if (!strcasecmp(name.c_str(), props[k])) g = k;
        if (g < 0) { why = "unknown configuration property '" + name + "'"; return false; }
        std::vector<std::string> tok;
        slist_split_tokens(val, 3, tok);
        // SLIST_3: fewer than three entries fail the config map's size check (src/flb_config_map.c:32-59) and the filter does not start
        if (tok.size() < 3) { why = name + " needs 'from_key to_key type': " + val; return false; }
        group[g].push_back(tok);
    }
    for (int g = 0; g < 4; g++) {
        for (const auto &tok : group[g]) {
            // a fourth entry, the rest of the line: config_rule's -1 (:74-79) is ignored by configure() (:121-132), the rule is skipped
            if (tok.size() != 3) continue;
            TRule r;
            r.src = src_of[g];
            // an unknown type word (flb_typecast_rule_create) and a from_key flb_ra_create refuses: config_rule frees the rule with
            // delete_conv_entry, which unlinks an entry that was never linked (:52, :95-100) -- the reference dies; refused here
            r.to = type_of_word(tok[2]);
            if (r.to < 0) { why = "unknown type word '" + tok[2] + "' (the reference does not survive it)"; return false; }
            r.from = tok[0]; r.to_key = tok[1];
            const int acc = accessor(tok[0], r.key, why);
            if (acc == ACC_REFUSE) return false;
            if (acc == ACC_SKIP) { why = "from_key '" + tok[0] + "': the record accessor refuses it (the reference does not survive it)"; return false; }
            r.inert = acc == ACC_INERT;
            if (r.inert) memset(&r.key, 0, sizeof(r.key));
            pg.rules.push_back(r);
        }
    }
    if (pg.rules.empty()) { why = "no rules"; return false; }           // (:134-137)
    if ((int) pg.rules.size() > TC_MAX_RULES) { why = "more than " + std::to_string(TC_MAX_RULES) + " rules"; return false; }
    std::vector<uint32_t> table;
    build_table(pg, table);
    if (table.size() * 4 > TC_MAX_TABLE_BYTES) { why = "rule table larger than " + std::to_string(TC_MAX_TABLE_BYTES) + " bytes"; return false; }
    return true;
}

std::string describe(const TProgram &pg) {
    static const char *const src[] = {"str", "int", "uint", "float"};
    static const char *const to[] = {"int", "uint", "float", "hex", "string", "bool"};
    std::string d;
    for (const TRule &r : pg.rules) {
        if (!d.empty()) d += ";";
        d += std::string(src[r.src]) + ">" + to[r.to] + ",";
        if (r.inert) d += "-";
        else {
            d += "K" + hexs(std::string(r.key.key, (size_t) r.key.key_len));
            for (int s = 0; s < r.key.nsub; s++) {
                if (r.key.sub_is_index[s]) d += "[" + std::to_string(r.key.sub_index[s]) + "]";
                else d += "." + hexs(std::string(r.key.sub_str + r.key.sub_off[s], (size_t) r.key.sub_len[s]));
            }
        }
        d += ",T" + hexs(r.to_key);
    }
    return d;
}

}  // namespace

// flb_ra_create(text, FLB_FALSE) as ra_parse_buffer cuts the text into parts (src/flb_record_accessor.c:74-230), in order
int flbgpu::ra_split(const std::string &a, std::vector<RaPart> &parts, std::string &why) {
    const long len = (long) a.size();
    auto string_part = [&](long from, long to) {
        RaPart p;
        p.kind = RA_STR;
        p.str = a.substr((size_t) from, (size_t) (to - from));
        parts.push_back(p);
    };
    long pre = 0, end = 0, i;
    for (i = 0; i < len; i++) {
        if (a[i] != '$') continue;
        if (i > pre) string_part(pre, i);
        pre = i;
        const long n = i + 1;
        if (n >= len) break;
        if (isdigit((unsigned char) a[n])) {                             // $0 .. $9: a regex id (atoi reads on, one digit is consumed)
            RaPart p;
            p.kind = RA_REGEX;
            p.id = atoi(a.c_str() + n);
            parts.push_back(p);
            i++;
            pre = i + 1;
            continue;
        }
        if (n + 2 < len && !a.compare(n, 3, "TAG")) {                    // $TAG, $TAG[n]
            if (n + 4 < len) {
                end = -1;
                if (a[n + 3] == '[') {
                    const long t = n + 3;
                    const size_t close = a.find(']', t);
                    end = close == std::string::npos ? -1 : (long) close - t;
                    if (end == 0) end = -1;
                    RaPart p;
                    p.kind = RA_TAGPART;
                    p.id = atoi(a.c_str() + t + 1);
                    parts.push_back(p);
                    i = t + end + 1;
                    pre = i;
                    continue;
                }
            }
            RaPart p;
            p.kind = RA_TAG;
            parts.push_back(p);
            i = n + 3;
            pre = n + 3;
            continue;
        }
        int quotes = 0;
        for (end = i + 1; end < len; end++) {
            const char c = a[end];
            if (c == '\'') quotes++;
            else if (c == '.' && (quotes & 1)) continue;
            else if (c == '.' || c == ' ' || c == ',' || c == '"') break;
        }
        RaPart p;
        p.kind = RA_KEY;
        std::string w2;
        if (!parse_ra(a.substr(i, end - i).c_str(), p.key, w2)) {
            if (w2 == "unterminated subkey string" || w2 == "bad subkey" || w2 == "trailing characters in record accessor") return RA_SPLIT_SKIP;
            why = w2;
            return RA_SPLIT_REFUSE;
        }
        parts.push_back(p);
        pre = end;
        i = end;
    }
    if ((i - 1 > end && pre < i) || i == 1) { if (pre < len) string_part(pre, len); }
    return RA_SPLIT_OK;
}

namespace {

bool front(int nprops, const char *const *names, const char *const *values, TProgram &pg) {
    return parse_front("type_converter", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, pg, why); });
}

struct TypeconvState : FilterState {
    struct Words { unsigned long long first_bad, counts[7]; };
    int nrules = 0;
    uint32_t table_bytes = 0;
    uint64_t done = 0, failed = 0, undefined = 0, mismatch = 0;        // since the filter was created (flbgpu_type_converter_counters)
    ScopedDevBuf d_table;
    CallWords<Words> words;
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

}  // namespace

extern "C" int flbgpu_type_converter_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    TProgram pg;
    if (!front(nprops, names, values, pg)) return -1;
    put_desc(desc, cap, describe(pg));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_type_converter_create(int nprops, const char *const *names, const char *const *values) {
    TProgram pg;
    if (!front(nprops, names, values, pg)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_TYPECONV;
    auto *m = new TypeconvState();
    f->state = m;
    m->nrules = (int) pg.rules.size();
    std::vector<uint32_t> table;
    build_table(pg, table);
    m->table_bytes = (uint32_t) (table.size() * 4);
    if (!filter_common_init(f) || !upload(m->d_table, table)) { delete f; return nullptr; }
    return f;
}

extern "C" void flbgpu_type_converter_counters(flbgpu_filter *f, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (auto *m = state_of<TypeconvState>(f, F_TYPECONV)) { out[0] = m->done; out[1] = m->failed; out[2] = m->undefined; out[3] = m->mismatch; }
}

// cb_type_converter_filter (:182-353) on a device chunk.  Every decoded record goes into the encoder, but the call hands the buffer
// on only when a conversion succeeded somewhere (:321-326) AND the decoder's loop ended on a clean end of data (:328-346): a record
// the decoder refuses, or undecodable bytes behind the rows (`garbage`), make the call answer NOTOUCH whatever was converted in front.
bool TypeconvState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) {
    const uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0) return true;
    if (!words.ensure() || !ensure_row_columns(f, n)) return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    TypeconvArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = table_bytes; a.nrules = nrules;
    a.len = f->d_len.as<uint32_t>();
    a.first_bad = &dw->first_bad; a.counts = dw->counts;
    auto size_pass = [&](const char *name) {
        return words.pass(f, st, name, [](Words &w) { memset(&w, 0, sizeof(w)); w.first_bad = ~0ull; }, [&] { launch_typeconv(a, false, st); });
    };
    if (!size_pass("k_typeconv(size)")) return false;
    const unsigned long long fb = hw.first_bad;
    if (fb == 0) return true;
    if (fb != ~0ull) {
        // the loop ends at the first record the decoder refuses: what the call converted is counted over the rows in front of it
        a.n = fb;
        if (!size_pass("k_typeconv(size, in front of a decoder error)")) return false;
    }
    done += hw.counts[2]; failed += hw.counts[3]; undefined += hw.counts[4];
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[0];
    if (fb != ~0ull || garbage) return true;                            // "Log event encoder error" (:341-346)
    if (hw.counts[5]) { set_err("filter_type_converter: a record's output is larger than 4 GB"); return false; }
    if (hw.counts[2] == 0 || hw.counts[1] == 0) return true;            // is_record_modified stayed false (:321-326)
    if (!scan_lengths(f, st, a.len, n, &words.total())) return false;
    a.out_off = f->d_off.as<uint64_t>(); a.out = f->d_out.as<uint8_t>();
    { ProfScope ps(f, st, "k_typeconv(emit)"); launch_typeconv(a, true, st); }
    HIPOK(hipMemcpyAsync(&hw.counts[6], &dw->counts[6], sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    mismatch += hw.counts[6];
    if (hw.counts[6]) { set_err("filter_type_converter: %llu rows were emitted with another length than they were sized", hw.counts[6]); return false; }
    set_out(f, out, n, words.total());
    f->last_out = hw.counts[1];
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
