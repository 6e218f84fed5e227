// throttle_sanitize.cpp -- a stand-alone driver for the host code of filter_throttle_size and filter_throttle under AddressSanitizer
// and UndefinedBehaviorSanitizer: flbgpu_throttle_size_parse_check and flbgpu_throttle_parse_check (csrc/throttle.cpp: what
// flb_utils_size_to_bytes, flb_utils_split, strtoul and both parse_duration accept, the raise of the duration, the path table) over
// every recorded property set (tests/golden/throttle_size_ref_cases.json, throttle_ref_cases.json, read with the few lines of JSON
// below) and over numbers, suffixes and paths at the parsers' edges.  It needs no device.  throttle.cpp and the filters' shared front
// (filter_host.cpp) are compiled into the program with the sanitizers; what they call outside themselves comes from the ordinary
// libflbgpu.so:
//
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -O1 -g -std=c++17 \
//       -o throttle_sanitize tools/throttle_sanitize.cpp fluent-bit_amd/csrc/throttle.cpp fluent-bit_amd/csrc/filter_host.cpp \
//       -Lfluent-bit_amd/csrc -lflbgpu -Wl,-rpath,$PWD/fluent-bit_amd/csrc
//   ./throttle_sanitize tests/golden/throttle_size_ref_cases.json tests/golden/throttle_ref_cases.json
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

extern "C" int flbgpu_throttle_size_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap);
extern "C" int flbgpu_throttle_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap);

typedef std::vector<std::pair<std::string, std::string>> Props;
static int g_ok = 0, g_refused = 0;

static void check(bool size, const Props &p) {
    std::vector<const char *> n, v;
    for (size_t i = 0; i < p.size(); i++) { n.push_back(p[i].first.c_str()); v.push_back(p[i].second.c_str()); }
    // the description into buffers of every size class: cut, never overrun
    for (size_t cap : {(size_t) 0, (size_t) 1, (size_t) 7, (size_t) 64, (size_t) 1 << 17}) {
        std::vector<char> desc(cap ? cap : 1);
        const int rc = (size ? flbgpu_throttle_size_parse_check : flbgpu_throttle_parse_check)((int) p.size(), n.data(), v.data(), cap ? desc.data() : nullptr, cap);
        if (cap == ((size_t) 1 << 17)) (rc == 0 ? g_ok : g_refused)++;
    }
}

// "props":[["name","value"],...] of every case: the strings between the quotes, JSON escapes undone as far as the generator writes them
static std::vector<Props> props_of(const char *path) {
    std::vector<Props> all;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::string s;
    char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, got);
    fclose(f);
    size_t at = 0;
    while ((at = s.find("\"props\":[", at)) != std::string::npos) {
        at += 9;
        Props p;
        std::vector<std::string> strs;
        int depth = 1;
        while (at < s.size() && depth > 0) {
            const char c = s[at++];
            if (c == '[') depth++;
            else if (c == ']') depth--;
            else if (c == '"') {
                std::string t;
                while (at < s.size() && s[at] != '"') {
                    if (s[at] == '\\' && at + 1 < s.size()) { at++; t.push_back(s[at] == 'n' ? '\n' : s[at] == 't' ? '\t' : s[at]); at++; }
                    else t.push_back(s[at++]);
                }
                at++;
                strs.push_back(t);
            }
        }
        for (size_t i = 0; i + 1 < strs.size(); i += 2) p.emplace_back(strs[i], strs[i + 1]);
        all.push_back(p);
    }
    return all;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++)
        for (const Props &p : props_of(argv[a])) check(strstr(argv[a], "throttle_size") != nullptr, p);
    const char *numbers[] = {"", "0", "1", "2", "-1", "1.5", "0.5", "1e3", "10x", "x", " 7", "7 ", "+3", "65536", "65537", "1k", "1K", "2kb", "1.5M", "1G", "3mb",
                             "1kx", "false", "1e400", "-1e400", "nan", "inf", "-inf", "0x10", "3s", "2m", "1h", "1d", "5ss", "1x", "s", "4294967297",
                             "99999999999999999999", "9223372036854775807", "9223372036854775.5k", "1e18G", "24855d", "24856d", "2147483647", "2147483648"};
    for (const char *v : numbers) {
        for (const char *n : {"rate", "window", "interval", "window_time_duration"}) check(true, {{n, v}});
        for (const char *n : {"rate", "window", "interval", "print_status"}) check(false, {{n, v}});
        check(true, {{"interval", v}, {"window", "65536"}});
    }
    std::string deep, wide(40000, 'x');
    for (int i = 0; i < 40; i++) deep += (i ? "|k" : "k") + std::to_string(i);
    for (const std::string &p : {std::string(""), std::string("|"), std::string("||"), std::string("a||b"), std::string("|a"), std::string("a||"), deep, deep + "||", wide,
                                 wide + "|" + wide}) {
        check(true, {{"name_field", p}});
        check(true, {{"log_field", p}, {"name_field", p}});
    }
    check(true, {});
    check(false, {});
    check(false, {{"rate", "2"}, {"rate", "3"}});
    check(false, {{"nope", "1"}});
    check(false, {{"interval", "${X}"}});
    printf("%d configurations accepted, %d refused\nclean\n", g_ok, g_refused);
    return 0;
}
