// rtag.cpp -- filter_rewrite_tag (plugins/filter_rewrite_tag/rewrite_tag.c): the configuration as the config map (:590-613) and
// process_config (:112-190) read it, the device program behind it, and one cb_rewrite_tag_filter call on a device chunk (:425-557)
// with the emitter's side of it (in_emitter_add_record, :403-420).  The per-record work is rtag_kernels.inc.
#include "filter_host.hpp"
#include "rtag.hpp"

using namespace flbgpu;

namespace {

struct RRule {
    std::string key_text, pattern, tag_text;
    bool keep = false, inert = false, needs_cap = false;
    uint32_t group_mask = 0;           // bit g: NEW_TAG reads `$g`
    DevKey key = {};
    std::vector<RaPart> parts;         // NEW_TAG
};
struct RProgram { std::vector<RRule> rules; };

void put_bytes(std::vector<uint32_t> &table, const char *s, size_t n) {
    for (size_t j = 0; j < n; j += 4) {
        uint32_t w = 0;
        for (size_t b = 0; b < 4 && j + b < n; b++) w |= (uint32_t) (unsigned char) s[j + b] << (8 * b);
        table.push_back(w);
    }
}

// a key's sub-key list (ra_lds.inc): two words per sub-key; returns its byte offset
uint32_t put_subs(std::vector<uint32_t> &table, const DevKey &k) {
    const size_t sub = table.size();
    table.resize(sub + 2 * (size_t) k.nsub, 0);
    for (int s = 0; s < k.nsub; s++) {
        if (k.sub_is_index[s]) { table[sub + 2 * s] = (uint32_t) k.sub_index[s] | 0x80000000u; continue; }
        table[sub + 2 * s] = (uint32_t) k.sub_len[s];
        table[sub + 2 * s + 1] = (uint32_t) (table.size() * 4);
        put_bytes(table, k.sub_str + k.sub_off[s], (size_t) k.sub_len[s]);
    }
    return (uint32_t) (sub * 4);
}

// the table of rtag.hpp
void build_table(const RProgram &pg, std::vector<uint32_t> &table) {
    table.assign(RT_RULE_WORDS * pg.rules.size(), 0);
    uint32_t ncap = 0;
    for (size_t i = 0; i < pg.rules.size(); i++) {
        const RRule &r = pg.rules[i];
        const uint32_t sub = put_subs(table, r.key);
        const uint32_t name = (uint32_t) (table.size() * 4);
        put_bytes(table, r.key.key, (size_t) r.key.key_len);
        const size_t parts = table.size();
        table.resize(parts + RT_PART_WORDS * r.parts.size(), 0);
        for (size_t k = 0; k < r.parts.size(); k++) {
            const RaPart &p = r.parts[k];
            uint32_t w0 = (uint32_t) p.kind, w1 = 0, w2 = 0, w3 = 0;
            if (p.kind == RA_STR) { w1 = (uint32_t) p.str.size(); w2 = (uint32_t) (table.size() * 4); put_bytes(table, p.str.data(), p.str.size()); }
            else if (p.kind == RA_TAGPART || p.kind == RA_REGEX) w1 = (uint32_t) p.id;
            else if (p.kind == RA_KEY) {
                w0 |= (uint32_t) p.key.nsub << 8;
                w3 = put_subs(table, p.key);
                w1 = (uint32_t) p.key.key_len; w2 = (uint32_t) (table.size() * 4);
                put_bytes(table, p.key.key, (size_t) p.key.key_len);
            }
            uint32_t *w = &table[parts + RT_PART_WORDS * k];
            w[0] = w0; w[1] = w1; w[2] = w2; w[3] = w3;
        }
        uint32_t *w = &table[RT_RULE_WORDS * i];
        w[0] = (r.keep ? RT_KEEP : 0u) | (r.inert ? RT_INERT : 0u) | (r.needs_cap ? RT_NEEDS_CAP : 0u) | ((uint32_t) r.key.nsub << 8) | ((uint32_t) r.parts.size() << 16);
        w[1] = (uint32_t) r.key.key_len; w[2] = name; w[3] = sub; w[4] = (uint32_t) (parts * 4);
        w[5] = r.needs_cap ? ncap++ : 0u;
    }
}

// a rule's pattern as flb_regex_create reads it (src/flb_regex.c:60-152), compiled for the device; false with `why`
bool compile_pattern(const RRule &r, bool numbered, rx::Program &prog, std::string &why) {
    const char *ps, *pe;
    unsigned opts;
    rx::split_flb_pattern(r.pattern.c_str(), &ps, &pe, &opts);
    std::string err;
    const bool ok = numbered ? rx::compile_numbered(ps, (size_t) (pe - ps), opts, r.group_mask, prog, err) : rx::compile(ps, (size_t) (pe - ps), opts, false, prog, err);
    if (ok) return true;
    // look-around, back-references, atomic groups ...: filter_grep hands such a rule to the host's backtracking matcher (rxbt.inc); this
    // filter needs the match -- and the spans -- where the tag is composed, on the device
    if (prog.nonregular) why = "Rule pattern '" + r.pattern + "' is not a regular expression (" + err + "): filter_rewrite_tag takes regular patterns only";
    else why = "could not compile regex pattern '" + r.pattern + "': " + err;
    return false;
}

// the config map (:590-613) and process_config (:112-190) over the properties in configuration order
bool parse_program(int nprops, const char *const *names, const char *const *values, RProgram &pg, std::string &why) {
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        if (!strcasecmp(name.c_str(), "emitter_name") || !strcasecmp(name.c_str(), "emitter_mem_buf_limit")) continue;
        if (!strcasecmp(name.c_str(), "emitter_storage.type")) {
            // cb_rewrite_tag_init (:281-286)
            if (strcasecmp(val.c_str(), "memory") && strcasecmp(val.c_str(), "filesystem")) {
                why = "invalid 'emitter_storage.type' value '" + val + "'. Only 'memory' or 'filesystem' types are allowed";
                return false;
            }
            continue;
        }
        if (strcasecmp(name.c_str(), "rule")) { why = "unknown configuration property '" + name + "'"; return false; }
        std::vector<std::string> tok;
        slist_split_tokens(val, 4, tok);
        // SLIST_4: fewer than four entries fail the config map's size check (src/flb_config_map.c:32-59); what follows the fourth
        // token is a fifth entry nobody reads (flb_slist_split_tokens with max_split 4)
        if (tok.size() < 4) { why = "Rule needs 'KEY REGEX NEW_TAG KEEP': " + val; return false; }
        RRule r;
        r.key_text = tok[0]; r.pattern = tok[1]; r.tag_text = tok[2];
        r.keep = !strcasecmp(tok[3].c_str(), "true") || !strcasecmp(tok[3].c_str(), "on") || !strcasecmp(tok[3].c_str(), "yes");   // flb_utils_bool == FLB_TRUE
        // KEY: flb_ra_regex_match reads the FIRST part, and only a part with a key finds anything
        std::vector<RaPart> kp;
        std::string w2;
        int rc = ra_split(r.key_text, kp, w2);
        if (rc == RA_SPLIT_SKIP) { why = "invalid record accessor key ? '" + r.key_text + "'"; return false; }
        if (rc == RA_SPLIT_REFUSE) { why = "Rule KEY '" + r.key_text + "': " + w2; return false; }
        if (kp.empty()) { why = "Rule KEY is empty (the reference reads the head of an empty part list)"; return false; }
        memset(&r.key, 0, sizeof(r.key));
        if (kp[0].kind == RA_KEY) r.key = kp[0].key;
        else if (kp[0].kind == RA_STR) {
            if (kp[0].str.size() >= (size_t) MAX_KEY) { why = "Rule KEY '" + r.key_text + "': key longer than " + std::to_string(MAX_KEY - 1) + " bytes"; return false; }
            r.key.is_ra = 1;
            memcpy(r.key.key, kp[0].str.data(), kp[0].str.size());
            r.key.key_len = (int) kp[0].str.size();
        }
        else r.inert = true;
        // NEW_TAG
        rc = ra_split(r.tag_text, r.parts, w2);
        if (rc == RA_SPLIT_SKIP) { why = "could not compose tag: " + r.tag_text; return false; }
        if (rc == RA_SPLIT_REFUSE) { why = "Rule NEW_TAG '" + r.tag_text + "': " + w2; return false; }
        if ((int) r.parts.size() > RT_MAX_PARTS) { why = "Rule NEW_TAG '" + r.tag_text + "': more than " + std::to_string(RT_MAX_PARTS) + " parts"; return false; }
        for (const RaPart &p : r.parts)
            if (p.kind == RA_REGEX) {
                r.needs_cap = true;
                if (p.id >= 0 && p.id <= 9) r.group_mask |= 1u << p.id;
            }
        rx::Program prog;
        if (!compile_pattern(r, false, prog, why)) return false;
        if (r.needs_cap) {
            rx::Program cp;
            if (!compile_pattern(r, true, cp, why)) return false;
            if (cp.ngroups > RT_MAX_GROUPS) { why = "Rule pattern '" + r.pattern + "': more than " + std::to_string(RT_MAX_GROUPS) + " capture groups"; return false; }
            // atoi reads `$12` as group 12 (src/flb_record_accessor.c:120-123): nothing where the pattern has no such group, as with the
            // reference; a pattern that HAS a tenth group and a template that reads it is past the ten span columns of a captured row
            for (const RaPart &p : r.parts)
                if (p.kind == RA_REGEX && p.id > 9 && p.id <= cp.ngroups) {
                    why = "Rule NEW_TAG '" + r.tag_text + "': regex id " + std::to_string(p.id) + " of a pattern with that many groups (only $0 .. $9 are kept)";
                    return false;
                }
        }
        pg.rules.push_back(r);
    }
    // no rule at all: the filter starts with a warning (:184-187) and every call answers NOTOUCH
    if ((int) pg.rules.size() > RT_MAX_RULES) { why = "more than " + std::to_string(RT_MAX_RULES) + " rules"; return false; }
    std::vector<uint32_t> table;
    build_table(pg, table);
    if (table.size() * 4 > RT_MAX_TABLE_BYTES) { why = "rule table larger than " + std::to_string(RT_MAX_TABLE_BYTES) + " bytes"; return false; }
    return true;
}

std::string describe_key(const DevKey &k) {
    std::string d = "K" + hexs(std::string(k.key, (size_t) k.key_len));
    for (int s = 0; s < k.nsub; s++) {
        if (k.sub_is_index[s]) d += "[" + std::to_string(k.sub_index[s]) + "]";
        else d += "." + hexs(std::string(k.sub_str + k.sub_off[s], (size_t) k.sub_len[s]));
    }
    return d;
}

std::string describe(const RProgram &pg) {
    std::string d;
    for (const RRule &r : pg.rules) {
        if (!d.empty()) d += ";";
        d += r.inert ? std::string("-") : describe_key(r.key);
        d += ",P" + hexs(r.pattern) + ",[";
        for (size_t k = 0; k < r.parts.size(); k++) {
            const RaPart &p = r.parts[k];
            if (k) d += " ";
            if (p.kind == RA_STR) d += "S" + hexs(p.str);
            else if (p.kind == RA_TAG) d += "T";
            else if (p.kind == RA_TAGPART) d += "t" + std::to_string(p.id);
            else if (p.kind == RA_REGEX) d += "R" + std::to_string(p.id);
            else d += describe_key(p.key);
        }
        d += std::string("],") + (r.keep ? "keep" : "drop");
    }
    return d;
}

bool front(int nprops, const char *const *names, const char *const *values, RProgram &pg) {
    return parse_front("rewrite_tag", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, pg, why); });
}

struct RtagState : FilterState {
    struct Words { unsigned long long first_bad, max_row, counts[6]; };
    struct Totals { uint64_t n_emit, tag_bytes, kept_bytes; unsigned long long kept; };
    int nrules = 0, ncaps = 0;
    uint32_t table_bytes = 0, max_vw = 0;                 // max_vw: widest position set of a capture program on the NFA engine (0: none)
    std::vector<std::unique_ptr<TableBlob>> blobs;
    ScopedDevBuf d_table, d_rules, d_caps, d_tag, d_rule, d_emit, d_emit_idx, d_taglen, d_tag_off, d_tags, d_table_out, d_spans, d_chk, d_refused;
    CallWords<Words, Totals> words;                       // (on the device, behind the words: the kept records' count of the last scan)
    std::string tag;
    bool tag_dirty = true;
    int (*emit_cb)(void *, const char *, int, const void *, size_t) = nullptr;
    void *emit_ctx = nullptr;
    uint64_t emitted = 0, refused = 0, mismatch = 0, tag_bytes = 0;      // since the filter was created (flbgpu_rewrite_tag_counters)
    // the last call's emissions
    uint64_t last_n = 0, last_tag_bytes = 0;              // on the device (every emission the kernels made)
    bool on_host = false;
    std::vector<RtagEmitted> h_recs;                      // on the host (the emissions the emitter took)
    std::vector<uint8_t> h_tags, h_input;
    const uint8_t *input = nullptr;
    uint64_t input_bytes = 0;
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

}  // namespace

extern "C" int flbgpu_rewrite_tag_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    RProgram pg;
    if (!front(nprops, names, values, pg)) return -1;
    put_desc(desc, cap, describe(pg));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_rewrite_tag_create(int nprops, const char *const *names, const char *const *values) {
    RProgram pg;
    std::string why;
    if (!front(nprops, names, values, pg)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_RTAG;
    auto *m = new RtagState();
    f->state = m;
    m->nrules = (int) pg.rules.size();
    std::vector<uint32_t> table;
    build_table(pg, table);
    m->table_bytes = (uint32_t) (table.size() * 4);
    std::vector<GrepRule> rules(pg.rules.size());
    std::vector<RtagCap> caps;
    for (size_t i = 0; i < pg.rules.size(); i++) {
        const RRule &r = pg.rules[i];
        memset(&rules[i], 0, sizeof(GrepRule));
        rx::Program prog;
        auto *b1 = new TableBlob(), *b2 = new TableBlob();
        m->blobs.emplace_back(b1); m->blobs.emplace_back(b2);
        if (!compile_pattern(r, false, prog, why) || !upload_dfa(prog.ascii, *b1, rules[i].dfa) || !upload_utf8(prog, *b2, rules[i].utf8)) {
            if (!why.empty()) set_err("filter_rewrite_tag: %s", why.c_str());
            delete f;
            return nullptr;
        }
        if (!r.needs_cap) continue;
        rx::Program cp;
        RtagCap c;
        memset(&c, 0, sizeof(c));
        auto *b3 = new TableBlob(), *b4 = new TableBlob();
        m->blobs.emplace_back(b3); m->blobs.emplace_back(b4);
        if (!compile_pattern(r, true, cp, why) || !upload_cap(cp.ascii, *b3, c.ascii) || !upload_utf8(cp, *b4, c.utf8)) {
            if (!why.empty()) set_err("filter_rewrite_tag: %s", why.c_str());
            delete f;
            return nullptr;
        }
        memset(c.slot2cap, 0xFF, sizeof(c.slot2cap));
        for (size_t s = 2; s < cp.slot2cap.size() && s < sizeof(c.slot2cap); s++) c.slot2cap[s] = cp.slot2cap[s] < RT_CAP_COLS ? cp.slot2cap[s] : 0xFF;
        c.ngroups = cp.ngroups;
        if (c.utf8.nfa_on && (uint32_t) c.utf8.nfa.VW > m->max_vw) m->max_vw = (uint32_t) c.utf8.nfa.VW;
        caps.push_back(c);
    }
    m->ncaps = (int) caps.size();
    f->rules = rules;                   // (flbgpu_filter_regex_corners reads the match tables' corner counters from here)
    if (!filter_common_init(f) || !upload(m->d_table, table) || !upload(m->d_rules, rules) || !upload(m->d_caps, caps)) { delete f; return nullptr; }
    return f;
}

extern "C" void flbgpu_rewrite_tag_set_tag(flbgpu_filter *f, const char *tag, int tag_len) {
    auto *m = state_of<RtagState>(f, F_RTAG);
    if (!m) return;
    m->tag.assign(tag && tag_len > 0 ? tag : "", tag && tag_len > 0 ? (size_t) tag_len : 0);
    m->tag_dirty = true;
}

extern "C" void flbgpu_rewrite_tag_set_emitter(flbgpu_filter *f, int (*emit)(void *ctx, const char *tag, int tag_len, const void *buf, size_t size), void *ctx) {
    if (auto *m = state_of<RtagState>(f, F_RTAG)) { m->emit_cb = emit; m->emit_ctx = ctx; }
}

extern "C" void flbgpu_rewrite_tag_counters(flbgpu_filter *f, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (auto *m = state_of<RtagState>(f, F_RTAG)) { out[0] = m->emitted; out[1] = m->refused; out[2] = m->mismatch; out[3] = m->tag_bytes; }
}

extern "C" int flbgpu_rewrite_tag_emitted(flbgpu_filter *f, flbgpu_rtag_emitted *out) {
    if (!out) return -1;
    memset(out, 0, sizeof(*out));
    RtagState *m = state_of<RtagState>(f, F_RTAG);
    if (!m) { set_err("filter_rewrite_tag: not a rewrite_tag filter"); return -1; }
    if (!m->on_host) {
        // a device-level call: every emission was taken; the table and the arena come over when somebody asks
        m->h_recs.resize(m->last_n);
        m->h_tags.resize(m->last_tag_bytes);
        if (m->last_n && hipMemcpy(m->h_recs.data(), m->d_table_out.p, m->last_n * sizeof(RtagEmitted), hipMemcpyDeviceToHost) != hipSuccess) { set_err("device read failed"); return -1; }
        if (m->last_tag_bytes && hipMemcpy(m->h_tags.data(), m->d_tags.p, m->last_tag_bytes, hipMemcpyDeviceToHost) != hipSuccess) { set_err("device read failed"); return -1; }
        m->on_host = true;
    }
    out->count = m->h_recs.size();
    out->recs = (const flbgpu_rtag_emitted_rec *) m->h_recs.data();
    out->tags = (const char *) m->h_tags.data();
    out->tag_bytes = m->h_tags.size();
    out->input = m->input;
    out->input_bytes = m->input_bytes;
    return 0;
}

extern "C" int flbgpu_rewrite_tag_emitted_dev(flbgpu_filter *f, flbgpu_rtag_emitted *out) {
    if (!out) return -1;
    memset(out, 0, sizeof(*out));
    RtagState *m = state_of<RtagState>(f, F_RTAG);
    if (!m) { set_err("filter_rewrite_tag: not a rewrite_tag filter"); return -1; }
    out->count = m->last_n;
    out->recs = m->last_n ? (const flbgpu_rtag_emitted_rec *) m->d_table_out.p : nullptr;
    out->tags = m->last_n ? (const char *) m->d_tags.p : nullptr;
    out->tag_bytes = m->last_tag_bytes;
    return 0;
}

static_assert(sizeof(RtagEmitted) == sizeof(flbgpu_rtag_emitted_rec), "the emitted table's entry is the C ABI's");

// cb_rewrite_tag_filter (:425-557) on a device chunk.  Launch order: match -> scan(emitted) -> size tags (capture walk) -> scan(tag
// bytes) -> write tags + table -> [host-level call: table and arena to the host, the emitter's answers, the refused rows' bitmap back] ->
// scan(kept bytes) -> copy.  The tags come before the compaction because a refusal changes what is kept; a call nobody refuses
// uploads nothing.  The call hands a buffer on only when a record was emitted (:517-522) AND the decoder's loop ended on a clean end of
// data (:533-551): the emissions in front of a decoder error have happened all the same.
bool RtagState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) {
    const uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    last_n = 0; last_tag_bytes = 0; on_host = true;
    h_recs.clear(); h_tags.clear(); input = nullptr; input_bytes = 0;
    if (n == 0) return true;
    if (!words.ensure(8)) return false;
    if (!d_rule.ensure(n * 4) || !d_emit.ensure(n * 4) || !d_taglen.ensure(n * 4) || !f->d_len.ensure(n * 4) ||
        !d_emit_idx.ensure((n + 1) * 8) || !d_tag_off.ensure((n + 1) * 8) || !f->d_off.ensure((n + 1) * 8) ||
        !f->d_scan_tmp.ensure(scan_tmp_elems(n) * sizeof(uint64_t)))
        return false;
    if (tag_dirty) {
        if (!d_tag.ensure(tag.size() + 16)) return false;
        if (!tag.empty()) HIPOK(hipMemcpyAsync(d_tag.p, tag.data(), tag.size(), hipMemcpyHostToDevice, st));
        HIPOK(hipStreamSynchronize(st));
        tag_dirty = false;
    }
    Words *dw = words.dev();
    Words &hw = words.host();
    Totals &tot = words.total();
    RtagArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = table_bytes; a.nrules = nrules;
    a.rules = d_rules.as<GrepRule>(); a.caps = d_caps.as<RtagCap>();
    a.tag = d_tag.as<uint8_t>(); a.tag_len = (uint32_t) tag.size();
    a.rule = d_rule.as<uint32_t>(); a.keep_len = f->d_len.as<uint32_t>(); a.emit = d_emit.as<uint32_t>();
    a.emit_idx = d_emit_idx.as<uint64_t>(); a.tag_lens = d_taglen.as<uint32_t>(); a.tag_off = d_tag_off.as<uint64_t>();
    a.first_bad = &dw->first_bad; a.counts = dw->counts;
    auto match_pass = [&](const char *name) {
        return words.pass(f, st, name, [](Words &w) { memset(&w, 0, sizeof(w)); w.first_bad = ~0ull; }, [&] { launch_rtag_match(a, st); });
    };
    if (!match_pass("k_rtag_match")) return false;
    const unsigned long long fb = hw.first_bad;
    if (fb == 0) return true;
    if (fb != ~0ull) {
        // the loop ends at the first record the decoder refuses: the rows in front of it are the call
        a.n = fb;
        if (!match_pass("k_rtag_match(in front of a decoder error)")) return false;
    }
    const uint64_t nn = a.n;
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[0];
    if (hw.counts[3]) { set_err("filter_rewrite_tag: a record is larger than 4 GB"); return false; }
    if (hw.counts[2] == 0) return true;                                 // nothing matched: emitted_num == 0 (:517-522)
    { ProfScope ps(f, st, "k_scan"); launch_scan(a.emit, nn, f->d_scan_tmp.as<uint64_t>(), d_emit_idx.as<uint64_t>(), st, nullptr); }
    if (ncaps) launch_max_row_len(in->row_off, nn, &dw->max_row, st);
    HIPOK(hipMemcpyAsync(&tot.n_emit, d_emit_idx.as<uint64_t>() + nn, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&hw.max_row, &dw->max_row, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const uint64_t n_emit = tot.n_emit;
    if (n_emit != hw.counts[2]) { set_err("filter_rewrite_tag: the emitted rows' scan disagrees with their count"); return false; }
    a.n_emit = n_emit;
    int waves = 65536 * (RT_BLOCK / 64);
    if (ncaps) {
        // the capture walk's scratch, per wave, as the parser's phase kernels size theirs (flbgpu.cpp run_generic): a state id every
        // CHK_STEP boundaries of the longest row; behind them the NFA engine's kept position sets where a rule's program runs on it
        uint32_t chk_len = (uint32_t) (hw.max_row / CHK_STEP) + 3;
        const uint32_t nfa_off = chk_len;
        if (max_vw) chk_len = nfa_off + 2u * (uint32_t) (hw.max_row / rx::NFA_CHK + 2) * (max_vw + 1) + 2;
        const int cus = device_cus() > 0 ? device_cus() : 256;
        waves = cus * 8 * (RT_BLOCK / 64);
        while (waves > RT_BLOCK / 64 && (size_t) waves * 64 * chk_len * sizeof(uint16_t) > ((size_t) 1 << 30)) waves /= 2;
        if (!d_chk.ensure((size_t) waves * 64 * chk_len * sizeof(uint16_t)) || !d_spans.ensure((size_t) RT_CAP_COLS * n_emit * 4 + 16)) return false;
        a.chk = d_chk.as<uint16_t>(); a.chk_len = chk_len; a.chk_nfa_off = nfa_off; a.spans = d_spans.as<uint32_t>();
    }
    { ProfScope ps(f, st, "k_rtag(size)"); launch_rtag(a, false, waves, st); }
    { ProfScope ps(f, st, "k_scan"); launch_scan(a.tag_lens, nn, f->d_scan_tmp.as<uint64_t>(), d_tag_off.as<uint64_t>(), st, nullptr); }
    HIPOK(hipMemcpyAsync(&tot.tag_bytes, d_tag_off.as<uint64_t>() + nn, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&hw, dw, sizeof(hw), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (hw.counts[3]) { set_err("filter_rewrite_tag: a tag is larger than 4 GB"); return false; }
    if (!d_tags.ensure(tot.tag_bytes + 16) || !d_table_out.ensure(n_emit * sizeof(RtagEmitted) + 16)) return false;
    a.tags = d_tags.as<uint8_t>(); a.table_out = d_table_out.as<RtagEmitted>();
    { ProfScope ps(f, st, "k_rtag(emit)"); launch_rtag(a, true, waves, st); }
    HIPOK(hipMemcpyAsync(&hw, dw, sizeof(hw), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (hw.counts[4] || hw.counts[3]) {
        mismatch += hw.counts[4];
        set_err("filter_rewrite_tag: %llu rows were written with another tag length than they were sized with (or their capture walk failed)", hw.counts[4]);
        return false;
    }
    last_n = n_emit; last_tag_bytes = tot.tag_bytes; on_host = false;
    uint64_t accepted = n_emit, n_ref = 0;
    if (f->rtag_host_call) {
        // the emitter's side: in_emitter_add_record per emission, in record order, on the caller's bytes
        h_recs.resize(n_emit);
        h_tags.resize(tot.tag_bytes);
        HIPOK(hipMemcpy(h_recs.data(), d_table_out.p, n_emit * sizeof(RtagEmitted), hipMemcpyDeviceToHost));
        if (tot.tag_bytes) HIPOK(hipMemcpy(h_tags.data(), d_tags.p, tot.tag_bytes, hipMemcpyDeviceToHost));
        if (in->data == f->rtag_dev_base && f->rtag_host_base) input = f->rtag_host_base;
        else {
            // behind another filter of a chain: that filter's output is this one's input, and it lives on the device
            h_input.resize(in->bytes);
            if (in->bytes) HIPOK(hipMemcpy(h_input.data(), in->data, in->bytes, hipMemcpyDeviceToHost));
            input = h_input.data();
        }
        input_bytes = in->bytes;
        on_host = true;
        if (emit_cb) {
            std::vector<uint32_t> bits((n_emit + 31) / 32, 0u);
            size_t w = 0;
            for (uint64_t e = 0; e < n_emit; e++) {
                const RtagEmitted &r = h_recs[e];
                const int rc = emit_cb(emit_ctx, (const char *) h_tags.data() + r.tag_off, (int) r.tag_len, input + r.in_off, r.len);
                if (rc < 0) { bits[e >> 5] |= 1u << (e & 31); n_ref++; }
                else h_recs[w++] = r;
            }
            h_recs.resize(w);
            accepted = n_emit - n_ref;
            if (n_ref) {
                if (!d_refused.ensure(bits.size() * 4)) return false;
                HIPOK(hipMemcpyAsync(d_refused.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, st));
                launch_rtag_refuse(a, d_refused.as<uint32_t>(), st);
                HIPOK(hipStreamSynchronize(st));
            }
        }
    }
    emitted += accepted; refused += n_ref; tag_bytes += hw.counts[5];
    if (accepted == 0) return true;                                     // emitted_num == 0 (:517-522)
    if (fb != ~0ull || garbage) return true;                            // "Log event encoder error" (:546-551)
    unsigned long long *d_kept = (unsigned long long *) (dw + 1);
    HIPOK(hipMemsetAsync(d_kept, 0, sizeof(unsigned long long), st));
    { ProfScope ps(f, st, "k_scan"); launch_scan(a.keep_len, n, f->d_scan_tmp.as<uint64_t>(), f->d_off.as<uint64_t>(), st, d_kept); }
    HIPOK(hipMemcpyAsync(&tot.kept_bytes, f->d_off.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&tot.kept, d_kept, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (!f->d_out.ensure(tot.kept_bytes + 16)) return false;
    GatherArgs ta;
    ta.data = (const uint8_t *) in->data; ta.row_off = in->row_off; ta.n = n; ta.keep_len = a.keep_len;
    ta.out_off = f->d_off.as<uint64_t>(); ta.out = f->d_out.as<uint8_t>(); ta.out_cap = 0;
    if (tot.kept_bytes) { ProfScope ps(f, st, "k_gather"); launch_gather(ta, st); }
    HIPOK(hipStreamSynchronize(st));
    set_out(f, out, n, tot.kept_bytes);
    f->last_out = tot.kept;
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
