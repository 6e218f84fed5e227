// nest.cpp -- filter_nest (plugins/filter_nest/nest.c): the configuration as configure() reads it (:57-175, behind the config map of
// :729-761), the device program behind it, and one cb_nest_filter call on a device chunk (:631-717).  The per-record work is
// nest_kernels.inc.
#include "filter_host.hpp"
#include "nest.hpp"

using namespace flbgpu;

namespace {

struct NWild { std::string key; bool prefix; };
struct NProgram {
    int op = 0;
    std::vector<NWild> wild;
    bool has_key = false;
    std::string key;
    bool add = false, remove = false;
    std::string prefix;
};

size_t pad4(size_t n) { return (n + 3) & ~(size_t) 3; }

// the config map (:729-761) and configure() (:57-175) over the properties in configuration order
bool parse_program(int nprops, const char *const *names, const char *const *values, NProgram &pg, std::string &why) {
    std::vector<std::string> once;
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        const char *n = name.c_str();
        // only Wildcard may repeat (FLB_CONFIG_MAP_MULT, :735-739): the config map refuses any other name that is set twice
        // (flb_config_map_properties_check, src/flb_config_map.c)
        if (strcasecmp(n, "wildcard")) {
            for (const std::string &o : once)
                if (!strcasecmp(o.c_str(), n)) { why = "configuration property '" + name + "' is set 2 times"; return false; }
            once.push_back(name);
        }
        if (!strcasecmp(n, "operation")) {
            // strncmp(val, "nest", 4): the first four bytes decide, with their case (:85-96)
            if (!strncmp(val.c_str(), "nest", 4)) pg.op = NEST_OP_NEST;
            else if (!strncmp(val.c_str(), "lift", 4)) pg.op = NEST_OP_LIFT;
            else { why = "Key \"operation\" has invalid value '" + val + "'. Expected 'nest' or 'lift'"; return false; }
        }
        else if (!strcasecmp(n, "wildcard")) {
            // (the reference reads key[-1] of an empty value, :115)
            if (val.empty()) { why = "Wildcard with an empty value"; return false; }
            NWild w;
            w.prefix = val.back() == '*';
            w.key = w.prefix ? val.substr(0, val.size() - 1) : val;
            pg.wild.push_back(w);
            if ((int) pg.wild.size() > NEST_MAX_WILDCARDS) { why = "more than " + std::to_string(NEST_MAX_WILDCARDS) + " Wildcard entries"; return false; }
        }
        else if (!strcasecmp(n, "nest_under") || !strcasecmp(n, "nested_under")) { pg.has_key = true; pg.key = val; }      // (:127-134)
        else if (!strcasecmp(n, "add_prefix")) { pg.prefix = val; pg.add = true; }
        else if (!strcasecmp(n, "remove_prefix")) { pg.prefix = val; pg.remove = true; }
        // (Prefix_with is known to configure(), :135-139, but not to the config map: the filter does not start)
        else { why = "unknown configuration property '" + name + "'"; return false; }
    }
    if (pg.add && pg.remove) { why = "Add_prefix and Remove_prefix are exclusive"; return false; }
    // (the reference reads ctx->operation as malloc left it, :161-165)
    if (!pg.op) { why = "Operation is missing"; return false; }
    size_t bytes = pad4(pg.key.size()) + pad4(pg.prefix.size());
    for (const NWild &w : pg.wild) bytes += pad4(w.key.size());
    if (bytes > NEST_MAX_KEY_BYTES) { why = "wildcards, key and prefix longer than " + std::to_string(NEST_MAX_KEY_BYTES) + " bytes together"; return false; }
    return true;
}

std::string describe(const NProgram &pg) {
    std::string d = pg.op == NEST_OP_NEST ? "nest" : "lift";
    d += pg.has_key ? ";K" + hexs(pg.key) : std::string(";K-");
    d += std::string(";P") + (pg.add ? "a" : pg.remove ? "r" : "n") + "," + hexs(pg.prefix);
    for (const NWild &w : pg.wild) d += std::string(";W") + (w.prefix ? "p" : "e") + "," + hexs(w.key);
    return d;
}

void put_bytes(std::vector<uint32_t> &table, const std::string &s) {
    for (size_t j = 0; j < s.size(); j += 4) {
        uint32_t w = 0;
        for (size_t b = 0; b < 4 && j + b < s.size(); b++) w |= (uint32_t) (unsigned char) s[j + b] << (8 * b);
        table.push_back(w);
    }
}

bool front(int nprops, const char *const *names, const char *const *values, NProgram &pg) {
    return parse_front("nest", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, pg, why); });
}

struct NestState : FilterState {
    struct Words { unsigned long long first_bad, counts[6]; };
    int op = 0, nwild = 0, has_key = 0, pfx = NEST_PFX_NONE;
    uint32_t table_bytes = 0, key_off = 0, key_len = 0, pfx_off = 0, pfx_len = 0;
    uint64_t modified = 0, overread = 0, undefined = 0, big = 0;        // since the filter was created (flbgpu_nest_counters)
    ScopedDevBuf d_table, d_mode;
    CallWords<Words> words;
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

}  // namespace

extern "C" int flbgpu_nest_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    NProgram pg;
    if (!front(nprops, names, values, pg)) return -1;
    put_desc(desc, cap, describe(pg));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_nest_create(int nprops, const char *const *names, const char *const *values) {
    NProgram pg;
    if (!front(nprops, names, values, pg)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_NEST;
    auto *m = new NestState();
    f->state = m;
    m->op = pg.op;
    m->nwild = (int) pg.wild.size();
    m->has_key = pg.has_key ? 1 : 0;
    m->pfx = pg.add ? NEST_PFX_ADD : pg.remove ? NEST_PFX_REMOVE : NEST_PFX_NONE;
    // the table (nest.hpp): the wildcards' lengths and offsets, their bytes, then the key and the prefix
    std::vector<uint32_t> table(2 * pg.wild.size());
    for (size_t i = 0; i < pg.wild.size(); i++) {
        table[2 * i] = (uint32_t) pg.wild[i].key.size() | (pg.wild[i].prefix ? NEST_PREFIX : 0u);
        table[2 * i + 1] = (uint32_t) (table.size() * 4);
        put_bytes(table, pg.wild[i].key);
    }
    m->key_off = (uint32_t) (table.size() * 4); m->key_len = (uint32_t) pg.key.size();
    put_bytes(table, pg.key);
    m->pfx_off = (uint32_t) (table.size() * 4); m->pfx_len = (uint32_t) pg.prefix.size();
    put_bytes(table, pg.prefix);
    m->table_bytes = (uint32_t) (table.size() * 4);
    if (!filter_common_init(f) || !upload(m->d_table, table)) { delete f; return nullptr; }
    return f;
}

extern "C" void flbgpu_nest_counters(flbgpu_filter *f, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (auto *m = state_of<NestState>(f, F_NEST)) { out[0] = m->modified; out[1] = m->overread; out[2] = m->undefined; out[3] = m->big; }
}

// cb_nest_filter (:631-717) on a device chunk.  A decoder error ends the loop and the call answers with what was encoded in front of
// it (:671-696) -- so undecodable bytes behind the rows (`garbage`) change nothing here.  MODIFIED whenever a byte came out (:698-711).
bool NestState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool) {
    const uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0) return true;
    if (!words.ensure() || !ensure_row_columns(f, n) || !d_mode.ensure(n)) return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    NestArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = table_bytes;
    a.op = op; a.nwild = nwild; a.has_key = has_key; a.key_off = key_off; a.key_len = key_len;
    a.pfx = pfx; a.pfx_off = pfx_off; a.pfx_len = pfx_len;
    a.len = f->d_len.as<uint32_t>(); a.mode = d_mode.as<uint8_t>();
    a.first_bad = &dw->first_bad; a.counts = dw->counts;
    auto size_pass = [&](const char *name) {
        return words.pass(f, st, name, [](Words &w) { memset(&w, 0, sizeof(w)); w.first_bad = ~0ull; }, [&] { launch_nest(a, false, st); });
    };
    if (!size_pass("k_nest(size)")) return false;
    const unsigned long long fb = hw.first_bad;
    if (fb == 0) return true;
    if (fb != ~0ull) {
        // the loop ends at the first record the decoder refuses: the call is the rows in front of it -- nothing is emitted for the
        // others, and the call-level facts are counted again over those rows only
        HIPOK(hipMemsetAsync(a.len + fb, 0, (n - fb) * sizeof(uint32_t), st));
        a.n = fb;
        if (!size_pass("k_nest(size, in front of a decoder error)")) return false;
    }
    modified += hw.counts[2]; big += hw.counts[3]; overread += hw.counts[4]; undefined += hw.counts[5];
    if (hw.counts[3]) { set_err("filter_nest: a record's output is larger than 4 GB"); return false; }
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[0];
    if (hw.counts[1] == 0) return true;                                 // nothing in the encoder: NOTOUCH (:706-711)
    if (!scan_lengths(f, st, a.len, n, &words.total())) return false;
    a.out_off = f->d_off.as<uint64_t>(); a.out = f->d_out.as<uint8_t>();
    { ProfScope ps(f, st, "k_nest(emit)"); launch_nest(a, true, st); }
    HIPOK(hipStreamSynchronize(st));
    set_out(f, out, n, words.total());
    f->last_out = hw.counts[1];
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
