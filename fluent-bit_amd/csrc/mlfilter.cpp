// mlfilter.cpp -- filter_multiline behind the C ABI (include/flb_gpu.h flbgpu_filter_multiline_create): mode parser with buffer off
// (plugins/filter_multiline/ml.c:224-446 cb_ml_init, :839-909 cb_ml_filter, the config map :992-1060).  The decoder loop hands every
// record to flb_ml_append_event on one stream, flb_ml_flush_pending_now flushes what is open: here one call takes all records of the
// chunk at once -- the records are the items of the multiline core (ml.cpp, ml_kernels.inc), mlfilter_kernels.inc builds the groups'
// records.  No CPU path.
#include "mlfilter.hpp"
#include "filter_host.hpp"

using namespace flbgpu;

namespace {
struct MlFilterState : FilterState {
    flbgpu_ml_parser *parser = nullptr;
    bool parser_owned = false;
    std::string parser_name, key;
    bool has_key = false;
    int nrules = 0;
    MlfStream stream;
    MlfTotals tot;
    ScopedDevBuf d_words, d_misc, d_keep, d_koff, d_ls, d_ll, d_irow, d_cls, d_tsec, d_tnsec, d_info, d_F, d_sin, d_act, d_c, d_coff, d_head, d_gidx, d_ghead,
           d_ovr, d_slow, d_fs_tmp, d_ev, d_evoff, d_regidx, d_plen, d_po, d_pre, d_dup, d_nrec, d_ridx, d_rows, d_carry;
    ~MlFilterState() override { if (parser && parser_owned) flbgpu_ml_parser_destroy(parser); }
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};
}  // namespace

namespace flbgpu {
uint64_t mlf_rows_of_call(uint64_t n, unsigned long long first_bad) { return first_bad == ~0ull || first_bad > n ? n : (uint64_t) first_bad; }

int mlf_round_step(uint64_t round, uint64_t items, unsigned long long trunc_k) {
    if (trunc_k == ~0ull) return MLF_ROUND_DONE;
    // every round pins one more item, so more rounds than items cannot be; MLF_TRUNC_ROUNDS bounds what a call may cost
    if (round >= (uint64_t) MLF_TRUNC_ROUNDS || round > items || trunc_k >= items) return MLF_ROUND_OVER;
    return MLF_ROUND_AGAIN;
}

int mlf_judge(const MlfWords &w, MlfTotals &t, std::string &why) {
    char b[256];
    if (w.meta_refused) {
        // flb_ml_stream_group_add_metadata's merge is not reproduced
        snprintf(b, sizeof(b), "%llu records of this chunk carry a non-empty metadata map: this call is not taken (keep it on the CPU path)", w.meta_refused);
        why = b; t.handed_back++;
        return MLF_HAND_BACK;
    }
    if (w.big) { why = "a record of this call is larger than 4 GB"; return MLF_FAIL; }
    if (w.empty_start) {
        // a start line without text opens a group that the next start joins instead of flushing it (flb_ml_rule.c:408-410): not reproduced
        snprintf(b, sizeof(b), "%llu records of this chunk start a group with an empty text: this call is not taken (keep it on the CPU path)", w.empty_start);
        why = b; t.handed_back++;
        return MLF_HAND_BACK;
    }
    if (w.mismatch) {
        snprintf(b, sizeof(b), "%llu records were written with another length than they were sized with", w.mismatch);
        why = b; t.mismatch += w.mismatch;
        return MLF_FAIL;
    }
    return MLF_GO;
}

void mlf_commit(MlfStream &s, MlfTotals &t, bool regex, uint32_t final_state, const MlfWords &w, uint64_t kept) {
    if (regex) s.state = final_state;
    if (w.has_reg) { s.sec = w.last_sec; s.nsec = w.last_nsec; }
    const uint64_t tr = w.truncated < kept ? (uint64_t) w.truncated : kept;
    t.truncations += tr;
    t.ok_records += kept - tr;
}
}  // namespace flbgpu

struct MlfConfig { std::string parser, key; bool has_key = false; };

static int utils_bool(const char *v) {          // flb_utils_bool
    if (!strcasecmp(v, "true") || !strcasecmp(v, "on") || !strcasecmp(v, "yes")) return 1;
    if (!strcasecmp(v, "false") || !strcasecmp(v, "off") || !strcasecmp(v, "no")) return 0;
    return -1;
}

// the config map and cb_ml_init's checks; what this project does not build is refused here
static bool parse_config(int nprops, const char *const *names, const char *const *values, MlfConfig &c, std::string &why) {
    static const char *known[] = {"debug_flush", "buffer", "mode", "flush_ms", "multiline.parser", "multiline.key_content", "emitter_name",
                                  "emitter_storage.type", "emitter_mem_buf_limit"};
    int buffer = 1;
    std::string mode = "parser";
    std::vector<std::string> parsers;
    for (int i = 0; i < nprops; i++) {
        bool ok = false;
        for (const char *k : known) ok = ok || !strcasecmp(names[i], k);
        if (!ok) { why = std::string("unknown property '") + names[i] + "'"; return false; }
        if (!strcasecmp(names[i], "buffer")) buffer = utils_bool(values[i]);
        else if (!strcasecmp(names[i], "mode")) mode = values[i];
        else if (!strcasecmp(names[i], "multiline.key_content")) { c.key = values[i]; c.has_key = true; }
        else if (!strcasecmp(names[i], "multiline.parser")) {
            const char *q = values[i];                  // a comma separated list (FLB_CONFIG_MAP_CLIST), blanks trimmed
            while (*q) {
                const char *e = strchr(q, ',');
                if (!e) e = q + strlen(q);
                const char *x = q, *y = e;
                while (x < y && *x == ' ') x++;
                while (y > x && y[-1] == ' ') y--;
                if (y > x) parsers.emplace_back(x, (size_t) (y - x));
                q = *e ? e + 1 : e;
            }
        }
    }
    if (strcasecmp(mode.c_str(), "parser") && strcasecmp(mode.c_str(), "partial_message")) { why = "'Mode' must be 'partial_message' or 'parser'"; return false; }
    if (!strcasecmp(mode.c_str(), "partial_message")) { why = "mode partial_message is not built"; return false; }
    if (buffer != 0) { why = "buffered mode is not built: say 'buffer off'"; return false; }
    if (parsers.empty()) { why = "mode parser requires at least one 'multiline.parser'"; return false; }
    if (parsers.size() > 1) { why = "more than one multiline parser is not built"; return false; }
    c.parser = parsers[0];
    if (c.has_key && c.key.size() > 255) { why = "multiline.key_content longer than 255 bytes"; return false; }
    return true;
}

static bool is_builtin(const std::string &n) { return n == "java" || n == "go" || n == "python" || n == "ruby"; }

// the parser the configuration names: the caller's definition, else a built-in.  *owned: created here
static flbgpu_ml_parser *resolve_parser(const MlfConfig &c, int nparsers, const char *const *parser_names, flbgpu_ml_parser *const *parsers, bool *owned, std::string &why) {
    *owned = false;
    if (c.parser == "docker" || c.parser == "cri") { why = "a multiline parser with a parser in front ('" + c.parser + "') is not built"; return nullptr; }
    for (int i = 0; i < nparsers; i++)
        if (parser_names && parser_names[i] && parsers && parsers[i] && c.parser == parser_names[i]) return parsers[i];
    if (!is_builtin(c.parser)) { why = "multiline parser '" + c.parser + "' is not defined"; return nullptr; }
    flbgpu_ml_parser *p = flbgpu_ml_parser_create("regex", nullptr, 0, "log", -1);
    if (!p) { why = flbgpu_last_error(); return nullptr; }
    if (flbgpu_ml_parser_builtin(p, c.parser.c_str()) != 0) { why = flbgpu_last_error(); flbgpu_ml_parser_destroy(p); return nullptr; }
    *owned = true;
    return p;
}

// (this front end reads every name and value as a C string: an entry without one is a bad argument too)
static bool null_entry(int nprops, const char *const *names, const char *const *values) {
    for (int i = 0; i < nprops; i++) if (!names[i] || !values[i]) return true;
    return false;
}

static const char *type_name(int t) { return t == ML_REGEX ? "regex" : t == ML_ENDSWITH ? "endswith" : "equal"; }

static bool build(int nprops, const char *const *names, const char *const *values, int nparsers, const char *const *parser_names,
                  flbgpu_ml_parser *const *parsers, MlFilterState *m, MlArgs &ma, std::string &why) {
    MlfConfig c;
    if (null_entry(nprops, names, values)) { why = "bad arguments"; return false; }
    if (!parse_config(nprops, names, values, c, why)) return false;
    bool owned = false;
    flbgpu_ml_parser *p = resolve_parser(c, nparsers, parser_names, parsers, &owned, why);
    if (!p) return false;
    m->parser = p; m->parser_owned = owned; m->parser_name = c.parser;
    std::string pkey;
    bool has_sub = false;
    memset(&ma, 0, sizeof(ma));
    if (!ml_parser_args(p, ma, pkey, has_sub, m->nrules)) { why = "multiline parser '" + c.parser + "' is not initialised"; return false; }
    if (has_sub) { why = "a multiline parser with a parser in front ('" + c.parser + "') is not built"; return false; }
    // "always override parent parser values" (multiline_load_parsers); a parser without key_content of its own then finds no content at all
    if (c.has_key) { m->key = c.key; m->has_key = true; }
    else if (!pkey.empty()) { m->key = pkey; m->has_key = true; }
    if (m->key.size() > 255) { why = "key_content longer than 255 bytes"; return false; }
    return true;
}

// host only: the device is not touched.  A name of parser_names counts as defined whether or not a handle comes with it (the
// definitions live on the device); a built-in is described from its table, never created
static bool describe(int nprops, const char *const *names, const char *const *values, int nparsers, const char *const *parser_names,
                     flbgpu_ml_parser *const *parsers, std::string &text, std::string &why) {
    MlfConfig c;
    if (null_entry(nprops, names, values)) { why = "bad arguments"; return false; }
    if (!parse_config(nprops, names, values, c, why)) return false;
    if (c.parser == "docker" || c.parser == "cri") { why = "a multiline parser with a parser in front ('" + c.parser + "') is not built"; return false; }
    int custom = -1;
    for (int i = 0; i < nparsers && custom < 0; i++) if (parser_names && parser_names[i] && c.parser == parser_names[i]) custom = i;
    if (custom < 0 && !is_builtin(c.parser)) { why = "multiline parser '" + c.parser + "' is not defined"; return false; }
    std::string key = c.has_key ? c.key : custom < 0 ? "log" : "";
    bool has_key = c.has_key || custom < 0;
    std::string extra;
    if (custom >= 0 && parsers && parsers[custom]) {
        MlArgs ma;
        std::string pkey;
        bool has_sub = false;
        int nrules = 0;
        memset(&ma, 0, sizeof(ma));
        if (!ml_parser_args(parsers[custom], ma, pkey, has_sub, nrules)) { why = "multiline parser '" + c.parser + "' is not initialised"; return false; }
        if (has_sub) { why = "a multiline parser with a parser in front ('" + c.parser + "') is not built"; return false; }
        if (!c.has_key && !pkey.empty()) { key = pkey; has_key = true; }
        char b[128];
        snprintf(b, sizeof(b), " type=%s rules=%d buffer_limit=%llu", type_name(ma.p.type), nrules, (unsigned long long) ma.p.buffer_limit);
        extra = b;
    }
    else if (custom < 0) {
        const int nr = c.parser == "java" || c.parser == "go" ? 8 : c.parser == "python" ? 4 : 2;
        char b[128];
        snprintf(b, sizeof(b), " type=regex rules=%d buffer_limit=%llu", nr, 2ull * 1024 * 1024);
        extra = b;
    }
    text = "parser=" + c.parser + " key_content=" + (has_key ? key : std::string("(none)")) + extra;
    return true;
}

extern "C" int flbgpu_multiline_parse_check(int nprops, const char *const *names, const char *const *values, int nparsers, const char *const *parser_names,
                                            flbgpu_ml_parser *const *parsers, char *desc, size_t cap) {
    std::string text;
    if (!parse_front("multiline", nprops, names, values, [&](std::string &why) { return describe(nprops, names, values, nparsers, parser_names, parsers, text, why); }))
        return -1;
    put_desc(desc, cap, text);
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_multiline_create(int nprops, const char *const *names, const char *const *values, int nparsers,
                                                         const char *const *parser_names, flbgpu_ml_parser *const *parsers) {
    auto *m = new MlFilterState();
    MlArgs ma;
    if (!parse_front("multiline", nprops, names, values, [&](std::string &why) { return build(nprops, names, values, nparsers, parser_names, parsers, m, ma, why); })) {
        delete m;
        return nullptr;
    }
    auto *f = new flbgpu_filter();
    f->kind = F_MLFILTER;
    f->state = m;
    if (!filter_common_init(f) || !m->d_carry.ensure(64)) { delete f; return nullptr; }
    return f;
}

extern "C" void flbgpu_multiline_counters(flbgpu_filter *f, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    auto *m = state_of<MlFilterState>(f, F_MLFILTER);
    if (!m) return;
    const MlfTotals &t = m->tot;
    out[0] = t.ok_records; out[1] = t.truncations; out[2] = t.handed_back; out[3] = t.mismatch;
}

extern "C" int flbgpu_multiline_state(flbgpu_filter *f) {
    auto *m = state_of<MlFilterState>(f, F_MLFILTER);
    return m ? (int) m->stream.state - 1 : -1;
}

// cb_ml_filter (:839-909) on a device chunk.  Launch order: class -> scan(rows handed out) -> items -> match -> fix -> [function scan ->
// act -> scans -> group heads -> first truncating continuation]* -> plan -> scan(registrations) -> their index -> size -> scans -> emit.
// The stream moves only when the call has succeeded.
bool MlFilterState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool) {
    // (`garbage` is not read: the decoder's loop simply ends at what it refuses, no clean-end check, :847-879)
    uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0) return true;
    if (in->bytes > 0xFFFF0000ull) { set_err("filter_multiline: more than 4 GB in one call"); return false; }
    if (!d_words.ensure(sizeof(MlfWords)) || !d_misc.ensure(sizeof(MlMisc)) || !d_keep.ensure(n * 4) || !d_koff.ensure((n + 1) * 8) ||
        !f->d_scan_tmp.ensure(scan_tmp_elems(2 * n + 2) * sizeof(uint64_t)))
        return false;
    MlfWords *dw = d_words.as<MlfWords>(), hw;
    uint64_t *tmp = f->d_scan_tmp.as<uint64_t>();
    MlfArgs a;
    memset(&a, 0, sizeof(a));
    MlArgs ma;
    memset(&ma, 0, sizeof(ma));
    std::string pkey;
    bool has_sub = false;
    int nrules = 0;
    if (!ml_parser_args(parser, ma, pkey, has_sub, nrules)) { set_err("filter_multiline: the parser is gone"); return false; }
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n; a.bytes = in->bytes;
    a.regex = ma.p.type == ML_REGEX ? 1u : 0u; a.type = (uint32_t) ma.p.type; a.match_len = ma.p.match_len;
    a.has_key = has_key ? 1u : 0u; a.key_len = (uint32_t) key.size();
    memcpy(a.key, key.data(), key.size());
    a.keep = d_keep.as<uint32_t>(); a.koff = d_koff.as<uint64_t>(); a.w = dw;
    a.carry_sec = stream.sec; a.carry_nsec = stream.nsec;
    uint64_t kept = 0;
    auto class_pass = [&]() {
        memset(&hw, 0, sizeof(hw));
        hw.first_bad = ~0ull;
        HIPOK(hipMemcpyAsync(dw, &hw, sizeof(hw), hipMemcpyHostToDevice, st));
        { ProfScope ps(f, st, "k_mlf_class"); launch_mlf_class(a, st); }
        { ProfScope ps(f, st, "k_scan"); launch_scan(a.keep, a.n, tmp, d_koff.as<uint64_t>(), st, nullptr); }
        HIPOK(hipMemcpyAsync(&hw, dw, sizeof(hw), hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(&kept, d_koff.as<uint64_t>() + a.n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        return true;
    };
    if (!class_pass()) return false;
    // the loop ends at the first record the decoder refuses: the rows in front of it are the call
    const uint64_t rows = mlf_rows_of_call(n, hw.first_bad);
    if (rows == 0) return true;
    if (rows != n) {
        a.n = n = rows;
        if (!class_pass()) return false;
    }
    std::string why;
    // (the words hold nothing but the metadata count yet) the call is handed back, the stream stays where it was
    auto judged = [&]() {
        const int j = mlf_judge(hw, tot, why);
        if (j != MLF_GO) set_err("filter_multiline: %s", why.c_str());
        if (j == MLF_HAND_BACK) *ret = -1;
        return j;
    };
    { const int j = judged(); if (j != MLF_GO) return j == MLF_HAND_BACK; }
    if (kept == 0) return true;
    const uint64_t N = kept + 1;
    a.N = N;
    if (!d_ls.ensure(N * 8) || !d_ll.ensure(N * 4) || !d_irow.ensure(N * 4) || !d_cls.ensure(N) || !d_tsec.ensure(N * 4) || !d_tnsec.ensure(N * 4) ||
        !d_info.ensure(N * 4) || !d_F.ensure(N * 8) || !d_sin.ensure(N) || !d_act.ensure(N) || !d_c.ensure(N * 4) || !d_coff.ensure((N + 1) * 8) ||
        !d_head.ensure(N * 4) || !d_gidx.ensure((N + 1) * 8) || !d_ghead.ensure((N + 1) * 8) || !d_ovr.ensure(N * 4) || !d_slow.ensure(N * 4) ||
        !d_fs_tmp.ensure(ml_fscan_tmp_bytes(N)) || !d_ev.ensure(2 * N * 4) || !d_evoff.ensure((2 * N + 1) * 8) || !d_regidx.ensure(2 * N * 4) ||
        !d_plen.ensure(N * 4) || !d_po.ensure((N + 1) * 8) || !d_pre.ensure(N * 4) || !d_dup.ensure(N * 4) || !d_nrec.ensure(N * 4) ||
        !d_ridx.ensure((N + 1) * 8))
        return false;
    a.ls = d_ls.as<uint64_t>(); a.ll = d_ll.as<uint32_t>(); a.irow = d_irow.as<uint32_t>(); a.cls = d_cls.as<uint8_t>();
    a.tsec = d_tsec.as<uint32_t>(); a.tnsec = d_tnsec.as<uint32_t>(); a.info = d_info.as<uint32_t>(); a.F = d_F.as<uint64_t>();
    a.act = d_act.as<uint8_t>(); a.c = d_c.as<uint32_t>(); a.coff = d_coff.as<uint64_t>(); a.head = d_head.as<uint32_t>();
    a.gidx = d_gidx.as<uint64_t>(); a.ghead = d_ghead.as<uint64_t>();
    a.ev = d_ev.as<uint32_t>(); a.evoff = d_evoff.as<uint64_t>(); a.regidx = d_regidx.as<uint32_t>();
    a.plen = d_plen.as<uint32_t>(); a.po = d_po.as<uint64_t>(); a.pre = d_pre.as<uint32_t>(); a.dup = d_dup.as<uint32_t>();
    a.nrec = d_nrec.as<uint32_t>(); a.ridx = d_ridx.as<uint64_t>();
    { ProfScope ps(f, st, "k_mlf_items"); launch_mlf_items(a, st); }
    // the multiline core on these items: item count N through koff[nl] + 1 with nl = 0, no carried bytes, every group closed by the flush
    MlMisc *dm = d_misc.as<MlMisc>(), hm;
    memset(&hm, 0, sizeof(hm));
    ma.p.has_key_content = 1;                    // breakline_prepare adds nothing while key_content is set
    ma.text = a.data; ma.bytes = in->bytes; ma.nl_pos = nullptr; ma.nl = 0; ma.koff = d_koff.as<uint64_t>() + n;
    ma.skip_empty_lines = 0; ma.flush_all = 1; ma.NB = N;
    ma.ls = a.ls; ma.ll = a.ll; ma.info = a.info; ma.F = a.F; ma.sin = d_sin.as<uint8_t>(); ma.act = d_act.as<uint8_t>();
    ma.c = d_c.as<uint32_t>(); ma.coff = a.coff; ma.head = d_head.as<uint32_t>(); ma.gidx = a.gidx; ma.ghead = d_ghead.as<uint64_t>();
    ma.ovr = d_ovr.as<uint32_t>(); ma.slow = d_slow.as<uint32_t>();
    ma.carry = d_carry.as<uint8_t>(); ma.carry_len = 0; ma.carry_tail = MLT_EMPTY; ma.carry_state = stream.state; ma.carry_trunc = 0;
    ma.misc = dm;
    HIPOK(hipMemsetAsync(dm, 0, sizeof(MlMisc), st));
    HIPOK(hipMemsetAsync(ma.ovr, 0xFF, N * 4, st));
    { ProfScope ps(f, st, "k_ml_match"); launch_ml_match(ma, device_cus() > 0 ? device_cus() : 256, st); }
    { ProfScope ps(f, st, "k_mlf_fix"); launch_mlf_fix(a, st); }
    const bool may_truncate = ma.p.type == ML_REGEX && ma.p.buffer_limit > 0;
    for (uint64_t round = 0;; round++) {
        // one truncating continuation is settled per round, exactly as flbgpu_ml_append_dev does (ml.cpp)
        launch_ml_reset(dm, st);
        launch_ml_fscan(ma.F, N, ma.p.type == ML_REGEX ? stream.state : (uint32_t) MLT_EMPTY, ma.sin, d_fs_tmp.p, &dm->final_state, st);
        { ProfScope ps(f, st, "k_ml_act"); launch_ml_act(ma, st); }
        launch_scan(ma.c, N, tmp, d_coff.as<uint64_t>(), st);
        launch_scan(ma.head, N, tmp, d_gidx.as<uint64_t>(), st);
        launch_ml_ghead(ma, st);
        if (may_truncate) launch_ml_trunc(ma, st);
        HIPOK(hipMemcpyAsync(&hm, dm, sizeof(hm), hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        const int step = mlf_round_step(round, N, hm.trunc_k);
        if (step == MLF_ROUND_DONE) break;
        if (step == MLF_ROUND_OVER) {
            set_err("filter_multiline: more than %d records of one call overflow buffer_limit (%llu bytes): this call is not taken", MLF_TRUNC_ROUNDS, (unsigned long long) ma.p.buffer_limit);
            return false;
        }
        launch_ml_override(ma, hm.trunc_k, st);
    }
    { ProfScope ps(f, st, "k_mlf_plan"); launch_mlf_plan(a, st); }
    launch_scan(a.ev, 2 * N, tmp, d_evoff.as<uint64_t>(), st);
    launch_mlf_regidx(a, st);
    { ProfScope ps(f, st, "k_mlf_size"); launch_mlf_size(a, st); }
    launch_scan(a.plen, N, tmp, d_po.as<uint64_t>(), st);
    launch_scan(a.nrec, N, tmp, d_ridx.as<uint64_t>(), st);
    uint64_t total = 0, R = 0;
    HIPOK(hipMemcpyAsync(&total, d_po.as<uint64_t>() + N, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&R, d_ridx.as<uint64_t>() + N, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&hw, dw, sizeof(hw), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    { const int j = judged(); if (j != MLF_GO) return j == MLF_HAND_BACK; }
    if (!f->d_out.ensure(total + 16) || !d_rows.ensure((R + 1) * 8)) return false;
    a.out = f->d_out.as<uint8_t>(); a.rows_out = d_rows.as<uint64_t>();
    { ProfScope ps(f, st, "k_mlf_emit"); launch_mlf_emit(a, st); }
    HIPOK(hipMemcpyAsync(&hw, dw, sizeof(hw), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (judged() != MLF_GO) return false;
    // the stream after the call
    mlf_commit(stream, tot, ma.p.type == ML_REGEX, hm.final_state, hw, kept);
    f->last_in = kept; f->last_out = R;
    if (total == 0) return true;
    out->data = f->d_out.p; out->row_off = d_rows.as<uint64_t>(); out->n = R; out->bytes = total;
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
