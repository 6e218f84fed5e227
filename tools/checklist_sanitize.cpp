// checklist_sanitize.cpp -- a stand-alone driver for the host code of filter_checklist under AddressSanitizer and
// UndefinedBehaviorSanitizer: flbgpu_checklist_parse_check (csrc/checklist.cpp: the front end and the list loader) over every
// recorded configuration with its list file (tests/golden/checklist_ref_cases.json, read with the few lines of JSON below) and over
// list files at the loader's edges -- lines of 2044 to 2047 bytes, a last line without a newline, NUL bytes anywhere.  It needs no
// device.  checklist.cpp and the filters' shared front (filter_host.cpp) are compiled into the program with the sanitizers; what they
// call outside themselves (the record accessor's parser, the token splitter) comes from the ordinary libflbgpu.so:
//
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -O1 -g -std=c++17 \
//       -o checklist_sanitize tools/checklist_sanitize.cpp fluent-bit_amd/csrc/checklist.cpp fluent-bit_amd/csrc/filter_host.cpp \
//       -Lfluent-bit_amd/csrc -lflbgpu -Wl,-rpath,$PWD/fluent-bit_amd/csrc
//   ./checklist_sanitize tests/golden/checklist_ref_cases.json
//
// It prints how many configurations were accepted and refused, and ends with "clean" and status 0; a sanitizer report ends it with
// another status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <utility>
#include <vector>

extern "C" int flbgpu_checklist_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap);

typedef std::vector<std::pair<std::string, std::string>> Props;

static std::string g_list_path, g_missing_path;

static int check(const Props &p, size_t cap) {
    std::vector<std::string> vals;
    for (const auto &kv : p) vals.push_back(kv.second == "@LIST@" ? g_list_path : kv.second == "@MISSING@" ? g_missing_path : kv.second);
    std::vector<const char *> n, v;
    for (size_t i = 0; i < p.size(); i++) { n.push_back(p[i].first.c_str()); v.push_back(vals[i].c_str()); }
    std::vector<char> desc(cap ? cap : 1);
    return flbgpu_checklist_parse_check((int) p.size(), n.data(), v.data(), cap ? desc.data() : nullptr, cap);
}

static void write_list(const std::string &bytes) {
    FILE *f = fopen(g_list_path.c_str(), "wb");
    if (!f) { perror(g_list_path.c_str()); exit(2); }
    if (!bytes.empty() && fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) { perror("fwrite"); exit(2); }
    fclose(f);
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

static std::string base64(const std::string &t) {
    std::string o;
    uint32_t acc = 0;
    int bits = 0;
    for (char c : t) {
        int v = c >= 'A' && c <= 'Z' ? c - 'A' : c >= 'a' && c <= 'z' ? c - 'a' + 26 : c >= '0' && c <= '9' ? c - '0' + 52 : c == '+' ? 62 : c == '/' ? 63 : -1;
        if (v < 0) continue;
        acc = (acc << 6) | (uint32_t) v;
        bits += 6;
        if (bits >= 8) { bits -= 8; o.push_back((char) ((acc >> bits) & 0xff)); }
    }
    return o;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: checklist_sanitize <tests/golden/checklist_ref_cases.json>\n"); return 2; }
    char dir[] = "/tmp/checklist_sanitize_XXXXXX";
    if (!mkdtemp(dir)) { perror("mkdtemp"); return 2; }
    g_list_path = std::string(dir) + "/list.txt";
    g_missing_path = std::string(dir) + "/no_such_file";
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
        const size_t l = text.find("\"list\":", i);
        if (l == std::string::npos) { fprintf(stderr, "case %d has no list\n", ncases); return 2; }
        i = l + 7;
        unlink(g_list_path.c_str());
        if (text[i] == '"') write_list(base64(json_string(text, i)));
        for (size_t cap : {(size_t) 0, (size_t) 1, (size_t) 17, (size_t) 1 << 17}) { if (check(p, cap) == 0) ok++; else refused++; }
        ncases++;
        pos = i;
    }
    if (ncases < 50) { fprintf(stderr, "only %d cases read from %s\n", ncases, argv[1]); return 2; }
    // ---- the loader's edges
    const std::string x2044(2044, 'x'), x2045(2045, 'x'), x2046(2046, 'x'), x2047(2047, 'x');
    const std::vector<std::string> lists = {
        "", "\n", "a", "a\n", "a\r\n", "a\r", "\r\n", "\r", "#\n", " #x\n", "a\n\nb\n", std::string("a\0b\n", 4), std::string("a\0b", 3),
        std::string("a\nb\0c\nd\n", 8), std::string("a\n\0", 3), std::string("\0", 1), std::string("a\n\0b\n", 5), std::string("\0\0\0", 3),
        x2044 + "\r\ny\n", x2045 + "\r\ny\n", x2045 + "\ny\n", x2046 + "\ny\n", x2046, x2045, "a\n" + x2046, "a\n" + x2047 + "\n", x2047,
        std::string(5000, 'x') + "\n", std::string(2046 * 3, 'x'), x2045 + std::string("\0", 1), std::string("\0", 1) + x2046, "A\xc9Z\n", "%\n_\n",
        x2045 + "\n" + x2045 + "\n" + x2045, std::string(100000, '\n'), std::string(4092, '#'),
    };
    for (const std::string &l : lists) {
        write_list(l);
        for (const char *fold : {"off", "on"}) for (const char *mode : {"exact", "partial"}) {
            if (check({{"file", "@LIST@"}, {"ignore_case", fold}, {"mode", mode}, {"record", "k v"}}, 1 << 12) == 0) ok++; else refused++;
        }
    }
    // ---- arguments
    if (flbgpu_checklist_parse_check(-1, nullptr, nullptr, nullptr, 0) == 0 || flbgpu_checklist_parse_check(1, nullptr, nullptr, nullptr, 0) == 0) return 2;
    { const char *nn[1] = {nullptr}, *vv[1] = {nullptr}; if (flbgpu_checklist_parse_check(1, nn, vv, nullptr, 0) == 0) return 2; }
    Props many;
    for (int i = 0; i < 65; i++) many.push_back({"record", "k" + std::to_string(i) + " v"});
    if (check(many, 1 << 12) == 0) return 2;
    if (check({{"record", "k " + std::string(70000, 'v')}}, 1 << 12) == 0) return 2;
    if (check({{"lookup_key", std::string(5000, 'k')}}, 1 << 12) == 0) return 2;
    unlink(g_list_path.c_str());
    rmdir(dir);
    printf("%d recorded configurations, %zu list files: %d answers accepted, %d refused\nclean\n", ncases, lists.size(), ok, refused);
    return 0;
}
