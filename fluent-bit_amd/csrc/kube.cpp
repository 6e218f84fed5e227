// kube.cpp -- filter_kubernetes (plugins/filter_kubernetes/kubernetes.c): the configuration as the config map (:905-1320) reads it, the
// cache entries flb_kube_meta_get (:692) would answer a hit with (lookup_pod_meta / lookup_namespace_meta, kube_meta.c:2463-2494; the
// properties array of flb_kube_prop_pack, kube_property.c:252-305), the pod entry of use_tag_for_meta (parse_regex_tag_data's tag
// branch and merge_meta_from_tag, kube_meta.c:1785-1811, 651-691, 1147-1200), and one cb_kube_filter call on a device chunk
// (:646-872).  The per-record work is kube_kernels.inc.  The metadata half -- the API server client -- is the caller's.
#include "filter_host.hpp"
#include "kube.hpp"

using namespace flbgpu;

namespace {

// kube_regex.h:25
const char KUBE_TAG_TO_REGEX[] = "(?<pod_name>[a-z0-9](?:[-a-z0-9]*[a-z0-9])?(?:\\.[a-z0-9](?:[-a-z0-9]*[a-z0-9])?)*)_(?<namespace_name>[^_]+)_(?<container_name>.+)-(?<docker_id>[a-z0-9]{64})\\.log$";

struct KProgram {
    bool merge_log = false, keep_log = true, trim = true, has_key = false, tag_meta = false;
    std::string merge_log_key, prefix = "kube.var.log.containers.";
};

// flb_utils_bool (src/flb_utils.c:757-771)
int bool_of(const std::string &v) {
    if (!strcasecmp(v.c_str(), "true") || !strcasecmp(v.c_str(), "on") || !strcasecmp(v.c_str(), "yes")) return 1;
    if (!strcasecmp(v.c_str(), "false") || !strcasecmp(v.c_str(), "off") || !strcasecmp(v.c_str(), "no")) return 0;
    return -1;
}

// the config map (:905-1320): the names that are read here or refused, then the ones that configure the metadata half (accepted and
// not looked at -- entries arrive finished), the FLB_CONFIG_MAP_BOOL ones apart: a bool that is none fails the check of the properties
const char *const BOOLS[] = {"merge_log", "keep_log", "merge_log_trim", "use_tag_for_meta", "use_journal", "dummy_meta", "tls.verify", "tls.verify_hostname",
                             "labels", "annotations", "owner_references", "namespace_labels", "namespace_annotations", "namespace_metadata_only",
                             "k8s-logging.parser", "k8s-logging.exclude", "cache_use_docker_id", "use_kubelet", "aws_use_pod_association",
                             "use_pod_association", "aws_pod_association_host_tls_verify"};
const char *const OTHERS[] = {"merge_log_key", "kube_tag_prefix", "merge_parser", "regex_parser", "buffer_size", "tls.debug", "tls.vhost", "kube_url",
                              "kube_meta_preload_cache_dir", "kube_ca_file", "kube_ca_path", "kube_namespace_file", "kube_token_file",
                              "kube_token_command", "dns_retries", "dns_wait_time", "kubelet_host", "kubelet_port", "kube_token_ttl",
                              "kube_meta_cache_ttl", "kube_meta_namespace_cache_ttl", "aws_pod_association_host", "aws_pod_association_endpoint",
                              "aws_pod_association_port", "aws_pod_service_map_ttl", "aws_pod_service_map_refresh_interval",
                              "aws_pod_service_preload_cache_dir", "aws_pod_association_host_server_ca_file",
                              "aws_pod_association_host_client_cert_file", "aws_pod_association_host_client_key_file",
                              "aws_pod_association_host_tls_debug", "set_platform"};

bool parse_program(int nprops, const char *const *names, const char *const *values, KProgram &pg, std::string &why) {
    std::vector<std::string> seen;
    for (int i = 0; i < nprops; i++) {
        const std::string name = names[i] ? names[i] : "", val = values[i] ? values[i] : "";
        const char *n = name.c_str();
        // (the engine translates ${VAR} in every value when the property is set: src/flb_filter.c flb_filter_set_property)
        if (val.find("${") != std::string::npos) { why = name + " '" + val + "': environment variables are not translated"; return false; }
        bool is_bool = false, known = false;
        for (const char *b : BOOLS) if (!strcasecmp(n, b)) is_bool = known = true;
        for (const char *o : OTHERS) if (!strcasecmp(n, o)) known = true;
        if (!known) { why = "unknown configuration property '" + name + "'"; return false; }
        // no property of this map has FLB_CONFIG_MAP_MULT: one that is set more than once fails the check (src/flb_config_map.c:551-560)
        for (const std::string &s : seen) if (!strcasecmp(s.c_str(), n)) { why = "configuration property '" + name + "' is set more than once"; return false; }
        seen.push_back(name);
        int b = 0;
        if (is_bool && (b = bool_of(val)) < 0) { why = "invalid boolean value '" + val + "' for '" + name + "'"; return false; }
        if (!strcasecmp(n, "merge_log")) pg.merge_log = b;
        else if (!strcasecmp(n, "keep_log")) pg.keep_log = b;
        else if (!strcasecmp(n, "merge_log_trim")) pg.trim = b;
        else if (!strcasecmp(n, "use_tag_for_meta")) pg.tag_meta = b;
        else if (!strcasecmp(n, "merge_log_key")) { pg.merge_log_key = val; pg.has_key = true; }
        else if (!strcasecmp(n, "kube_tag_prefix")) pg.prefix = val;
        else if (!strcasecmp(n, "use_journal")) { if (b) { why = "use_journal: the metadata is per record there (not built)"; return false; } }
        else if (!strcasecmp(n, "dummy_meta")) { if (b) { why = "dummy_meta: its metadata is the wall clock (not built)"; return false; } }
        else if (!strcasecmp(n, "merge_parser") || !strcasecmp(n, "regex_parser")) { why = name + " names a parser of a registry that does not exist here"; return false; }
    }
    if (pg.merge_log_key.size() >= KB_MAX_MERGE_KEY) { why = "merge_log_key of " + std::to_string(KB_MAX_MERGE_KEY) + " bytes or more"; return false; }
    return true;
}

std::string describe(const KProgram &pg) {
    return std::string("merge_log=") + (pg.merge_log ? "1" : "0") + ";keep_log=" + (pg.keep_log ? "1" : "0") + ";trim=" + (pg.trim ? "1" : "0") +
           ";merge_log_key=" + (pg.has_key ? hexs(pg.merge_log_key) : std::string("-")) + ";tag_meta=" + (pg.tag_meta ? "1" : "0") + ";prefix=" + hexs(pg.prefix);
}

bool checked_program(int nprops, const char *const *names, const char *const *values, KProgram &pg) {
    return parse_front("kubernetes", nprops, names, values, [&](std::string &why) { return parse_program(nprops, names, values, pg, why); });
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

// one msgpack object at d[p..len): p moves behind it.  false: truncated, the reserved byte, or a 33rd open container (msgpack_unpack_next
// would not answer it).  what: the first byte's family -- 'n' nil, 'b' bool, 's' STR, 'a' ARRAY, 'o' anything else
bool mp_object(const uint8_t *d, size_t len, size_t &p, int depth, char *what = nullptr, uint64_t *count = nullptr) {
    if (p >= len) return false;
    const uint8_t c = d[p++];
    uint64_t n = 0, pay = 0, kids = 0;
    int lb = 0;
    char w = 'o';
    if (c <= 0x7f || c >= 0xe0) {}
    else if (c >= 0xa0 && c <= 0xbf) { pay = c & 31; w = 's'; }
    else if (c >= 0x90 && c <= 0x9f) { kids = c & 15; w = 'a'; }
    else if (c >= 0x80 && c <= 0x8f) { kids = 2 * (uint64_t) (c & 15); w = 'm'; }
    else switch (c) {
        case 0xc0: w = 'n'; break;
        case 0xc1: return false;
        case 0xc2: case 0xc3: w = 'b'; break;
        case 0xc4: case 0xc7: case 0xd9: lb = 1; break;
        case 0xc5: case 0xc8: case 0xda: case 0xdc: case 0xde: lb = 2; break;
        case 0xc6: case 0xc9: case 0xdb: case 0xdd: case 0xdf: lb = 4; break;
        case 0xca: case 0xce: case 0xd2: pay = 4; break;
        case 0xcb: case 0xcf: case 0xd3: pay = 8; break;
        case 0xcc: case 0xd0: pay = 1; break;
        case 0xcd: case 0xd1: pay = 2; break;
        default: pay = (1ull << (c - 0xd4)) + 1; break;            // fixext 1 .. 16: the type byte and the data
    }
    if (lb) {
        if (len - p < (size_t) lb) return false;
        for (int i = 0; i < lb; i++) n = (n << 8) | d[p++];
        if (c >= 0xdc) { kids = c >= 0xde ? 2 * n : n; w = c >= 0xde ? 'm' : 'a'; }
        else { pay = n + (c >= 0xc7 && c <= 0xc9 ? 1 : 0); if (c >= 0xd9) w = 's'; }
    }
    if (len - p < pay) return false;
    p += pay;
    if (w == 'a' || w == 'm') {
        if (depth >= 32) return false;
        if (count) *count = w == 'a' ? kids : kids / 2;
        for (uint64_t i = 0; i < kids; i++) if (!mp_object(d, len, p, depth + 1)) return false;
    }
    if (what) *what = w;
    return true;
}

struct KubeState : FilterState {
    struct Words { unsigned long long firsts[2], counts[8]; };
    KProgram pg;
    std::vector<uint32_t> table;
    // the entries' first objects as they are appended, and what the properties array says
    std::string pod, ns;
    bool excl_stdout = false, excl_stderr = false;
    std::vector<uint8_t> tail;
    uint32_t tail_pairs = 0, lds_budget = KB_LDS_BLOB_DEFAULT;
    bool tail_in_lds = false, dirty = true;
    bool tag_failed = false;              // use_tag_for_meta: no tag yet, or the last set_tag failed (:700-702)
    rx::BtProgram *tag_rx = nullptr;
    uint64_t merged = 0, excluded = 0, odd = 0, mismatch = 0;             // since the filter was created (flbgpu_kubernetes_counters)
    ScopedDevBuf d_table, d_tail, d_state;
    CallWords<Words> words;
    ~KubeState() override { if (tag_rx) rx::bt_free(tag_rx); }
    void build();
    bool place();
    bool run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) override;
};

// the LDS table of kube.hpp and the tail every record ends on (:586-637)
void KubeState::build() {
    tail.clear();
    tail_pairs = 0;
    auto add = [&](const char *key, const std::string &blob) {
        if (blob.empty()) return;
        const std::string k = packed_str(key);
        tail.insert(tail.end(), k.begin(), k.end());
        tail.insert(tail.end(), blob.begin(), blob.end());
        tail_pairs++;
    };
    add("kubernetes", pod);
    add("kubernetes_namespace", ns);
    tail_in_lds = !tail.empty() && tail.size() <= lds_budget;
    const std::string mk = pg.has_key ? packed_str(pg.merge_log_key) : std::string();
    table.assign(KB_HDR_WORDS, 0);
    table[0] = (pg.merge_log ? KBF_MERGE_LOG : 0) | (pg.keep_log ? KBF_KEEP_LOG : 0) | (pg.trim ? KBF_TRIM : 0) | (pg.has_key ? KBF_MERGE_KEY : 0) |
               (excl_stdout ? KBF_EXCL_STDOUT : 0) | (excl_stderr ? KBF_EXCL_STDERR : 0) | (tail_pairs << KBF_TAIL_PAIRS_SHIFT);
    table[1] = (uint32_t) mk.size();
    table[2] = (uint32_t) tail.size();
    table[3] = tail_in_lds ? 1 : 0;
    for (size_t j = 0; j < mk.size(); j += 4) {
        uint32_t w = 0;
        for (size_t b = 0; b < 4 && j + b < mk.size(); b++) w |= (uint32_t) (unsigned char) mk[j + b] << (8 * b);
        table.push_back(w);
    }
    dirty = true;
}

bool KubeState::place() {
    if (!dirty) return true;
    if (!upload(d_table, table) || !upload(d_tail, tail)) { set_err("filter_kubernetes: the metadata could not be placed on the device"); return false; }
    dirty = false;
    return true;
}

// the first object of a cache entry; behind the pod's, optionally, the properties array.  false: refused (why)
bool read_entry(const uint8_t *d, size_t len, bool with_props, std::string &first, bool &ex_out, bool &ex_err, std::string &why) {
    first.clear();
    ex_out = ex_err = false;
    if (!d || !len) return true;
    if (len > KB_MAX_ENTRY) { why = "an entry over 1 MiB"; return false; }
    size_t p = 0;
    if (!mp_object(d, len, p, 0)) { why = "the entry's first object does not decode"; return false; }
    first.assign((const char *) d, p);
    if (!with_props || p == len) return true;
    // flb_kube_prop_unpack (kube_property.c:310-357): [stdout_parser | nil, stderr_parser | nil, stdout_exclude, stderr_exclude]
    size_t q = p;
    char w = 0;
    uint64_t cnt = 0;
    if (!mp_object(d, len, q, 0, &w, &cnt) || w != 'a' || cnt != 4) { why = "the properties array has another shape"; return false; }
    q = p + (d[p] == 0xdc ? 3 : d[p] == 0xdd ? 5 : 1);
    for (int i = 0; i < 4; i++) {
        const uint8_t c = d[q];
        if (!mp_object(d, len, q, 1, &w)) { why = "the properties array has another shape"; return false; }
        if (i < 2) {
            if (w == 's') { why = "a parser name in the properties: there is no parser registry here"; return false; }
            if (w != 'n') { why = "the properties array has another shape"; return false; }
        }
        else {
            if (w != 'b') { why = "the properties array has another shape"; return false; }
            (i == 2 ? ex_out : ex_err) = c == 0xc3;
        }
    }
    return true;
}

}  // namespace

static rx::BtProgram *tag_pattern();

extern "C" int flbgpu_kubernetes_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap) {
    KProgram pg;
    if (!checked_program(nprops, names, values, pg)) return -1;
    put_desc(desc, cap, describe(pg));
    return 0;
}

extern "C" flbgpu_filter *flbgpu_filter_kubernetes_create(int nprops, const char *const *names, const char *const *values) {
    KProgram pg;
    if (!checked_program(nprops, names, values, pg)) return nullptr;
    auto *f = new flbgpu_filter();
    f->kind = F_KUBE;
    auto *m = new KubeState();
    f->state = m;
    m->pg = pg;
    m->tag_failed = pg.tag_meta;
    // the test switch: a lower budget for the tail in LDS, so that both paths of the append are met with blobs of a few bytes
    if (const char *e = getenv("FLBGPU_KUBE_LDS_BLOB")) {
        char *end = nullptr;
        const unsigned long v = strtoul(e, &end, 10);
        if (end != e && v < m->lds_budget) m->lds_budget = (uint32_t) v;
    }
    if (pg.tag_meta) {
        m->tag_rx = tag_pattern();
        if (!m->tag_rx) { delete f; return nullptr; }
    }
    m->build();
    if (!filter_common_init(f) || !m->place()) {
        set_err("filter_kubernetes: the configuration could not be placed on the device");
        delete f;
        return nullptr;
    }
    return f;
}

extern "C" int flbgpu_kubernetes_set_meta(flbgpu_filter *f, const void *pod_entry, size_t pod_len, const void *ns_entry, size_t ns_len) {
    KubeState *m = state_of<KubeState>(f, F_KUBE);
    if (!m) { set_err("filter_kubernetes: not a kubernetes filter"); return -1; }
    std::string pod, ns, why;
    bool eo = false, ee = false, x = false, y = false;
    if (!read_entry((const uint8_t *) pod_entry, pod_entry ? pod_len : 0, true, pod, eo, ee, why)) { set_err("filter_kubernetes: pod entry: %s", why.c_str()); return -1; }
    if (!read_entry((const uint8_t *) ns_entry, ns_entry ? ns_len : 0, false, ns, x, y, why)) { set_err("filter_kubernetes: namespace entry: %s", why.c_str()); return -1; }
    m->pod = pod; m->ns = ns; m->excl_stdout = eo; m->excl_stderr = ee;
    m->build();
    return m->place() ? 0 : -1;
}

// parse_regex_tag_data's tag branch, cb_results and merge_meta_from_tag: the pod entry of a tag.  false: last_error says why
static bool tag_to_entry(const std::string &prefix, const rx::BtProgram *tag_rx, const char *tag, int tag_len, std::string &pod) {
    if (!tag || tag_len < 0) { set_err("filter_kubernetes: bad arguments"); return false; }
    const int plen = (int) prefix.size();
    if (plen + 1 >= tag_len) { set_err("filter_kubernetes: incoming record tag is shorter than kube_tag_prefix"); return false; }
    const int ng = rx::bt_ngroups(tag_rx);
    std::vector<int> beg((size_t) ng + 1, -1), end((size_t) ng + 1, -1);
    const int r = rx::bt_search(tag_rx, (const uint8_t *) tag + plen, tag_len - plen, beg.data(), end.data());
    if (r == -4) { set_err("filter_kubernetes: the backtrack budget was spent on the tag"); return false; }
    if (r <= 0) { set_err("filter_kubernetes: invalid pattern for given tag"); return false; }
    static const char *const fields[] = {"pod_name", "namespace_name", "container_name", "docker_id"};
    const auto &nm = rx::bt_names(tag_rx);
    const auto &groups = rx::bt_name_groups(tag_rx);
    std::string body;
    uint32_t n = 0;
    for (const char *fld : fields) {
        for (size_t i = 0; i < nm.size(); i++) {
            if (nm[i] != fld || groups[i].empty()) continue;
            const int g = groups[i].back();
            if (g > ng || beg[(size_t) g] < 0 || end[(size_t) g] <= beg[(size_t) g]) break;           // (vlen == 0: not taken)
            body += packed_str(fld) + packed_str(std::string(tag + plen + beg[(size_t) g], (size_t) (end[(size_t) g] - beg[(size_t) g])));
            n++;
            break;
        }
    }
    // flb_mp_map_header_init / _end: a map32 header whatever the count
    pod.clear();
    pod.push_back((char) 0xdf);
    for (int i = 3; i >= 0; i--) pod.push_back((char) (n >> (8 * i)));
    pod += body;
    return true;
}

static rx::BtProgram *tag_pattern() {
    std::string err;
    rx::BtProgram *p = rx::bt_compile(KUBE_TAG_TO_REGEX, sizeof(KUBE_TAG_TO_REGEX) - 1, 0, err);
    if (!p) set_err("filter_kubernetes: the tag pattern does not compile: %s", err.c_str());
    return p;
}

extern "C" int flbgpu_kubernetes_set_tag(flbgpu_filter *f, const char *tag, int tag_len) {
    KubeState *m = state_of<KubeState>(f, F_KUBE);
    if (!m) { set_err("filter_kubernetes: not a kubernetes filter"); return -1; }
    if (!m->pg.tag_meta) { set_err("filter_kubernetes: set_tag needs use_tag_for_meta on"); return -1; }
    m->tag_failed = true;
    std::string pod;
    if (!tag_to_entry(m->pg.prefix, m->tag_rx, tag, tag_len, pod)) return -1;
    m->pod = pod;
    m->ns.clear();
    m->excl_stdout = m->excl_stderr = false;
    m->build();
    if (!m->place()) return -1;
    m->tag_failed = false;
    return 0;
}

extern "C" int flbgpu_kubernetes_tag_check(int nprops, const char *const *names, const char *const *values, const char *tag, int tag_len, char *desc, size_t cap) {
    KProgram pg;
    if (!checked_program(nprops, names, values, pg)) return -1;
    if (!pg.tag_meta) { set_err("filter_kubernetes: set_tag needs use_tag_for_meta on"); return -1; }
    rx::BtProgram *p = tag_pattern();
    if (!p) return -1;
    std::string pod;
    const bool ok = tag_to_entry(pg.prefix, p, tag, tag_len, pod);
    rx::bt_free(p);
    if (!ok) return -1;
    put_desc(desc, cap, hexs(pod));
    return 0;
}

extern "C" int flbgpu_kubernetes_meta_check(const void *pod_entry, size_t pod_len, const void *ns_entry, size_t ns_len, char *desc, size_t cap) {
    std::string pod, ns, why;
    bool eo = false, ee = false, x = false, y = false;
    if (!read_entry((const uint8_t *) pod_entry, pod_entry ? pod_len : 0, true, pod, eo, ee, why)) { set_err("filter_kubernetes: pod entry: %s", why.c_str()); return -1; }
    if (!read_entry((const uint8_t *) ns_entry, ns_entry ? ns_len : 0, false, ns, x, y, why)) { set_err("filter_kubernetes: namespace entry: %s", why.c_str()); return -1; }
    put_desc(desc, cap, "pod=" + (pod.empty() ? std::string("-") : hexs(pod)) + ";ns=" + (ns.empty() ? std::string("-") : hexs(ns)) +
             ";stdout_exclude=" + (eo ? "1" : "0") + ";stderr_exclude=" + (ee ? "1" : "0"));
    return 0;
}

extern "C" void flbgpu_kubernetes_counters(flbgpu_filter *f, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (auto *m = state_of<KubeState>(f, F_KUBE)) { out[0] = m->merged; out[1] = m->excluded; out[2] = m->odd; out[3] = m->mismatch; }
}

extern "C" void flbgpu_kubernetes_layout(flbgpu_filter *f, uint64_t out[3]) {
    out[0] = out[1] = out[2] = 0;
    if (auto *m = state_of<KubeState>(f, F_KUBE)) {
        out[0] = m->tail.size(); out[1] = m->tail_in_lds ? 1 : 0;
        out[2] = m->table.size() * 4 + (m->tail_in_lds ? m->tail.size() : 0);
    }
}

// cb_kube_filter (:646-872) on a device chunk.  Once the metadata step answered the call is MODIFIED: every record the decoder hands on
// is built again -- [[EventTime, {}], body] -- unless the pod's properties exclude its stream; the loop ends at the first record the
// decoder refuses and hands on what stands in front of it (:733, :863-871).  A time the encoder refuses ends the call as NOTOUCH
// (:398-400, :822-834), and so does a failed set_tag (:700-702).
bool KubeState::run(flbgpu_filter *f, const flbgpu_dev_chunk *in, flbgpu_dev_chunk *out, hipStream_t st, int *ret, bool garbage) {
    (void) garbage;
    uint64_t n = in->n;
    *ret = FLBGPU_FILTER_NOTOUCH;
    f->last_in = 0; f->last_out = 0;
    if (n == 0 || tag_failed) return true;
    if (!place() || !words.ensure() || !ensure_row_columns(f, n) || !d_state.ensure(n)) return false;
    Words *dw = words.dev();
    Words &hw = words.host();
    uint64_t &total = words.total();
    KubeArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *) in->data; a.row_off = in->row_off; a.n = n;
    a.table = d_table.as<uint32_t>(); a.table_bytes = (uint32_t) (table.size() * 4);
    a.tail = d_tail.as<uint8_t>(); a.tail_bytes = (uint32_t) tail.size(); a.tail_in_lds = tail_in_lds ? 1 : 0;
    a.state = d_state.as<uint8_t>(); a.len = f->d_len.as<uint32_t>();
    a.firsts = dw->firsts; a.counts = dw->counts;
    auto size = [&](const char *name) {
        // the rows the first instantiation defers are sized by the exact one behind it (most calls have none: it reads the state column)
        return words.pass(f, st, name, [](Words &w) { memset(w.firsts, 0xff, sizeof(w.firsts)); memset(w.counts, 0, sizeof(w.counts)); },
                          [&] { launch_kube(a, KB_SIZE, false, st); launch_kube(a, KB_SIZE, true, st); });
    };
    if (!size("k_kube(size)")) return false;
    // a record the encoder refuses the time of, in front of anything the decoder refuses: the call hands back nothing
    if (hw.firsts[1] != ~0ull && hw.firsts[1] < hw.firsts[0]) return true;
    if (hw.firsts[0] != ~0ull) {
        a.n = n = hw.firsts[0];
        if (n == 0) { memset(out, 0, sizeof(*out)); *ret = FLBGPU_FILTER_MODIFIED; return true; }
        if (!size("k_kube(size, in front of a decoder error)")) return false;
    }
    if (hw.counts[5]) { set_err("filter_kubernetes: a record is larger than 4 GB"); return false; }
    f->last_in = hw.counts[0];
    f->last_out = hw.counts[4];
    const uint64_t c_merged = hw.counts[1], c_excl = hw.counts[2], c_odd = hw.counts[3], c_defer = hw.counts[7];
    if (!scan_lengths(f, st, a.len, n, &total)) return false;
    if (total == 0) {                                                    // every record excluded, group markers only: an empty buffer
        merged += c_merged; excluded += c_excl; odd += c_odd;
        memset(out, 0, sizeof(*out));
        *ret = FLBGPU_FILTER_MODIFIED;
        return true;
    }
    a.out_off = f->d_off.as<uint64_t>(); a.out = f->d_out.as<uint8_t>();
    { ProfScope ps(f, st, "k_kube(emit)"); launch_kube(a, KB_EMIT, false, st); if (c_defer) launch_kube(a, KB_EMIT, true, st); }
    HIPOK(hipMemcpyAsync(&hw.counts[6], &dw->counts[6], sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    mismatch += hw.counts[6];
    if (hw.counts[6]) { set_err("filter_kubernetes: %llu rows were emitted with another length than they were sized", hw.counts[6]); return false; }
    merged += c_merged; excluded += c_excl; odd += c_odd;
    set_out(f, out, n, total);
    *ret = FLBGPU_FILTER_MODIFIED;
    return true;
}
