// expect_sanitize.cpp -- a stand-alone driver for the host code of filter_expect under AddressSanitizer and
// UndefinedBehaviorSanitizer: flbgpu_expect_parse_check and flbgpu_expect_text_check (csrc/expect.cpp: the front end, the rule table,
// the messages) over every recorded configuration (tests/golden/expect_ref_cases.json, read with the few lines of JSON below) and over
// rule values at the splitter's edges -- spaces only, one word, words behind runs of spaces, accessors cut anywhere, the caps of the
// rule count, the table and the result key.  It needs no device.  expect.cpp and the filters' shared front (filter_host.cpp) are
// compiled into the program with the sanitizers; what they call outside themselves (the record accessor's parser) comes from the
// ordinary libflbgpu.so:
//
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -O1 -g -std=c++17 \
//       -o expect_sanitize tools/expect_sanitize.cpp fluent-bit_amd/csrc/expect.cpp fluent-bit_amd/csrc/filter_host.cpp \
//       -Lfluent-bit_amd/csrc -lflbgpu -Wl,-rpath,$PWD/fluent-bit_amd/csrc
//   ./expect_sanitize tests/golden/expect_ref_cases.json
//
// It prints how many configurations were accepted and refused, and ends with "clean" and status 0; a sanitizer report ends it with
// another status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

extern "C" int flbgpu_expect_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap);
extern "C" int flbgpu_expect_text_check(int nprops, const char *const *names, const char *const *values, uint64_t rule, uint32_t kind, uint32_t vtype,
                                        const void *val, size_t val_len, char *buf, size_t cap);

typedef std::vector<std::pair<std::string, std::string>> Props;

static int g_texts = 0;

static int check(const Props &p, size_t cap) {
    std::vector<const char *> n, v;
    for (size_t i = 0; i < p.size(); i++) { n.push_back(p[i].first.c_str()); v.push_back(p[i].second.c_str()); }
    std::vector<char> desc(cap ? cap : 1);
    const int rc = flbgpu_expect_parse_check((int) p.size(), n.data(), v.data(), cap ? desc.data() : nullptr, cap);
    if (rc != 0) return rc;
    // every message of every rule (and of one rule too many), into buffers of every size class
    const std::string val("va\0lue", 6);
    for (uint64_t rule = 0; rule <= p.size(); rule++)
        for (uint32_t kind = 0; kind <= 5; kind++)
            for (uint32_t vt : {0u, 4u, 6u, 9u}) {
                std::vector<char> buf(cap ? cap : 1);
                if (flbgpu_expect_text_check((int) p.size(), n.data(), v.data(), rule, kind, vt, kind == 4 ? val.data() : nullptr, kind == 4 ? val.size() : 0,
                                             cap ? buf.data() : nullptr, cap) >= 0) g_texts++;
            }
    return 0;
}

// a JSON string at s[i] == '"': its value; i ends behind the closing quote (the fixture holds ASCII and \uXXXX below 0x100 only)
static std::string json_string(const std::string &s, size_t &i) {
    std::string o;
    for (i++; i < s.size() && s[i] != '"'; i++) {
        if (s[i] != '\\') { o.push_back(s[i]); continue; }
        i++;
        if (s[i] == 'u') { o.push_back((char) strtol(s.substr(i + 1, 4).c_str(), nullptr, 16)); i += 4; }
        else o.push_back(s[i] == 'n' ? '\n' : s[i] == 't' ? '\t' : s[i] == 'r' ? '\r' : s[i]);
    }
    i++;
    return o;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: expect_sanitize <tests/golden/expect_ref_cases.json>\n"); return 2; }
    int ok = 0, refused = 0, ncases = 0;
    // ---- the recorded configurations, one case a line
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::string text;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
    fclose(f);
    size_t pos = 0;
    while ((pos = text.find("\"props\":[", pos)) != std::string::npos) {
        size_t i = pos + 9;
        Props p;
        while (i < text.size() && text[i] == '[') {                     // ["name","value"]
            i++;
            std::string k = json_string(text, i);
            i++;                                                        // ,
            std::string v = json_string(text, i);
            i++;                                                        // ]
            if (text[i] == ',') i++;
            p.emplace_back(k, v);
        }
        for (size_t cap : {(size_t) 0, (size_t) 1, (size_t) 17, (size_t) 1 << 17}) { if (check(p, cap) == 0) ok++; else refused++; }
        ncases++;
        pos = i;
    }
    if (ncases < 100) { fprintf(stderr, "only %d cases read from %s\n", ncases, argv[1]); return 2; }
    // ---- the splitter's and the accessor's edges
    const std::vector<std::string> values = {
        "", " ", "   ", "k", " k", "k ", " k ", "k v", "k  v", "  k   v  ", "k v w", "k v  w  ", "$", "$ ", " $", "$$", "$k", "$k v", "$k['a']", "$k['a'] v",
        "$k['a", "$k['a v", "$k[", "$k[1", "$k[1]", "$k[1]['b'][2] v", "$k[x]", "$k['a']x", "$k['a''b']", "$k.a", "$k.a v", "a.b", "a$b", "a$b c", "$TAG", "$TAG[1]",
        "$TAG[", "$0", "$9 v", "${", "${X}", "k ${X}", "$k[99999999999999999999]", std::string(127, 'k'), std::string(128, 'k'), "$" + std::string(127, 'k'),
        "$" + std::string(128, 'k'), "k " + std::string(70000, 'v'), std::string(70000, ' ') + "k", "$k['" + std::string(5000, 'a') + "']", "k\tv", "\"k v\" w",
    };
    const char *const rules[] = {"key_exists", "key_not_exists", "key_val_is_null", "key_val_is_not_null", "key_val_eq", "action", "result_key", "KEY_VAL_EQ", "nope"};
    for (const std::string &v : values)
        for (const char *r : rules) { if (check({{r, v}}, 1 << 12) == 0) ok++; else refused++; }
    // ---- arguments and caps
    if (flbgpu_expect_parse_check(-1, nullptr, nullptr, nullptr, 0) == 0 || flbgpu_expect_parse_check(1, nullptr, nullptr, nullptr, 0) == 0) return 2;
    { const char *nn[1] = {nullptr}, *vv[1] = {nullptr}; if (flbgpu_expect_parse_check(1, nn, vv, nullptr, 0) == 0) return 2; }
    Props many;
    for (int i = 0; i < 64; i++) many.push_back({"key_val_eq", "$k" + std::to_string(i) + "['s'][" + std::to_string(i) + "] v" + std::to_string(i)});
    if (check(many, 1 << 17) != 0) return 2;
    many.push_back({"result_key", "r"});
    if (check(many, 1 << 17) != 0) return 2;
    many.push_back({"action", "exit"});
    if (check(many, 1 << 17) == 0) return 2;
    if (check({{"result_key", std::string(65535, 'r')}}, 1 << 12) == 0 || check({{"result_key", std::string(65536, 'r')}}, 1 << 12) == 0) return 2;
    if (check({{"result_key", std::string(30000, 'r')}, {"action", "result_key"}}, 1 << 12) != 0) return 2;
    if (check({{"key_val_eq", "k " + std::string(32768 - 16 - 8 - 32 - 4, 'v')}}, 1 << 12) != 0) return 2;
    if (check({{"key_val_eq", "k " + std::string(32769 - 16 - 8 - 32 - 4, 'v')}}, 1 << 12) == 0) return 2;
    printf("%d recorded configurations, %zu rule values: %d answers accepted, %d refused, %d messages\nclean\n", ncases, values.size(), ok, refused, g_texts);
    return 0;
}
