// rtag_sanitize.cpp -- a stand-alone driver for the host code of filter_rewrite_tag under AddressSanitizer and
// UndefinedBehaviorSanitizer: flbgpu_rewrite_tag_parse_check (csrc/rtag.cpp) over the front-end cases, the accessor splitter that moved
// out of typeconv.cpp's private part (ra_split, reached through both filters' parse checks) and the two number formats a tag is
// composed with, "%ld" and "%f" (csrc/numconv_host.cpp), over the number edges.  It needs no device.  rtag.cpp, typeconv.cpp, the filters'
// shared front (filter_host.cpp) and numconv_host.cpp are compiled into the program with the sanitizers; what they call outside themselves (the regex compiler, the
// record accessor's parser, the token splitter) comes from the ordinary libflbgpu.so:
//
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -O1 -g -std=c++17 \
//       -o rtag_sanitize tools/rtag_sanitize.cpp fluent-bit_amd/csrc/rtag.cpp fluent-bit_amd/csrc/typeconv.cpp \
//       fluent-bit_amd/csrc/filter_host.cpp fluent-bit_amd/csrc/numconv_host.cpp -Lfluent-bit_amd/csrc -lflbgpu -Wl,-rpath,$PWD/fluent-bit_amd/csrc
//   ./rtag_sanitize
//
// It prints how many configurations were accepted and refused and how many numbers went through, and ends with "clean" and status 0;
// a sanitizer report ends it with another status.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

extern "C" {
int flbgpu_rewrite_tag_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap);
int flbgpu_type_converter_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap);
int flbgpu_nc_fmt_f6(double v, char *buf, int cap);
int flbgpu_nc_fmt_ld(long long v, char *buf);
}

typedef std::vector<std::pair<std::string, std::string>> Props;

static int check(const Props &p, size_t cap, bool typeconv = false) {
    std::vector<const char *> n, v;
    for (const auto &kv : p) { n.push_back(kv.first.c_str()); v.push_back(kv.second.c_str()); }
    std::vector<char> desc(cap ? cap : 1);
    return (typeconv ? flbgpu_type_converter_parse_check : flbgpu_rewrite_tag_parse_check)((int) p.size(), n.data(), v.data(), cap ? desc.data() : nullptr, cap);
}

int main() {
    const std::vector<std::string> keys = {"log", "$log", "$a['b']", "$a['b'][2]", "$a[0]", "pre$x", "$TAG", "$TAG[1]", "$TAG[", "$TAG[]", "$3", "$", "$$", "a.b", "$a.b",
                                           "$a['x", "$a[y]", "$a[' ", "$a[99999999999999999999]", "$9z", "", "\"\"", "$-a", "$" + std::string(127, 'k'),
                                           "$" + std::string(128, 'k'), std::string(127, 'k'), std::string(128, 'k'), std::string(5000, 'k') + "$a",
                                           "$a['" + std::string(256, 's') + "']", "$a['" + std::string(257, 's') + "']", "$a['it''s']", "$a['x.y']"};
    const std::vector<std::string> pats = {"^x$", ".", "(a)(b)?", "^(?<n>\\d+)-(\\w+)$", "/^ab/i", "/x/", "/", "//", "(", "[z", "(?=a)b", "(a)\\1", "(?>x)", "(?<!x)y",
                                           "\\d{2,3}", "(x)(x)(x)(x)(x)(x)(x)(x)(x)(x)", "[[:alpha:]]+", "é+"};
    const std::vector<std::string> tags = {"t", "\"\"", "$TAG", "$TAG[0].$TAG[12]", "$TAG[", "$TAG[]", "$TAG[x]", "$TAG[-1]", "$TAGS", "$TA", "$0$1$2", "$10", "$99999999999",
                                           "x$", "$", "$k.$k['a'][0],$j", "$k['x", "$k[x]", "a.$k.b", "$k,$k,$k,$k,$k,$k,$k,$k", "$k,$k,$k,$k,$k,$k,$k,$k,$k",
                                           std::string(5000, 'x'), std::string(30000, 'x'), "$" + std::string(128, 'k'), "$k" + std::string("['s']['s']['s']['s']['s']['s']['s']['s']['s']")};
    const std::vector<std::string> keeps = {"true", "false", "ON", "off", "yes", "no", "x", "\"\"", "true and more", ""};
    std::vector<Props> progs = {{}, {{"emitter_name", "e"}}, {{"emitter_storage.type", "memory"}}, {{"Emitter_Storage.Type", "FILESYSTEM"}}, {{"emitter_storage.type", "disk"}},
                                {{"emitter_mem_buf_limit", "10M"}}, {{"bogus", "1"}}, {{"", ""}}, {{"Rule", ""}}, {{"Rule", "   "}}, {{"Rule", "a"}}, {{"Rule", "a b"}},
                                {{"Rule", "a b c"}}, {{"Rule", "\"a b c d"}}, {{"Rule", "a \"b\\\" c\" d true"}}, {{"Rule", "a b c \""}}};
    for (const std::string &k : keys) progs.push_back({{"Rule", k + " ^x$ t true"}});
    for (const std::string &p : pats) { progs.push_back({{"Rule", "$k " + p + " t.$1 true"}}); progs.push_back({{"Rule", "$k " + p + " t false"}}); }
    for (const std::string &t : tags) { progs.push_back({{"Rule", "$k (a)(b) " + t + " true"}}); progs.push_back({{"Rule", "$k a " + t + " false"}}); }
    for (const std::string &w : keeps) progs.push_back({{"RULE", "$k a t " + w}});
    {
        Props p32, p33;
        for (int i = 0; i < 33; i++) {
            const std::string r = "k" + std::to_string(i) + " ^v" + std::to_string(i) + "$ t" + std::to_string(i) + ".$TAG.$1 true";
            if (i < 32) p32.push_back({"Rule", r});
            p33.push_back({"Rule", r});
        }
        progs.push_back(p32); progs.push_back(p33);
        progs.push_back({{"Rule", "abcd . " + std::string(24576 - 24 - 4 - 16, 't') + " true"}});
        progs.push_back({{"Rule", "abcd . " + std::string(24577 - 24 - 4 - 16, 't') + " true"}});
    }
    int ok = 0, refused = 0;
    for (const Props &p : progs)
        for (size_t cap : {(size_t) 0, (size_t) 1, (size_t) 2, (size_t) 17, (size_t) 1 << 17}) { if (check(p, cap) == 0) ok++; else refused++; }
    if (flbgpu_rewrite_tag_parse_check(-1, nullptr, nullptr, nullptr, 0) == 0 || flbgpu_rewrite_tag_parse_check(1, nullptr, nullptr, nullptr, 0) == 0) return 2;
    { const char *n[1] = {nullptr}, *v[1] = {nullptr}; if (flbgpu_rewrite_tag_parse_check(1, n, v, nullptr, 0) == 0) return 2; }
    printf("front end: %d answers accepted, %d refused\n", ok, refused);
    // the splitter through the filter it moved out of: every key text as a from_key
    int tok = 0, tref = 0;
    for (const std::string &k : keys) { if (check({{"str_key", k + " t int"}}, 64, true) == 0) tok++; else tref++; }
    for (const std::string &t : tags) { if (check({{"str_key", t + " t int"}}, 64, true) == 0) tok++; else tref++; }
    printf("splitter through filter_type_converter: %d accepted, %d refused\n", tok, tref);

    // ---- numbers: "%f" into a buffer of exactly the cap it is given, "%ld" into one of exactly its 20 characters
    const uint64_t fbits[] = {0, 0x8000000000000000ull, 0x3ff0000000000000ull, 0xbff8000000000000ull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
                              0x7ff8000000000000ull, 0xfff8000000000123ull, 1, 0x7fefffffffffffffull, 0xffefffffffffffffull, 0x444b1ae4d6e2ef50ull,
                              0x3fb999999999999aull, 0x7e37e43c8800759cull, 0x4480f0cf064dd592ull, 0x44b52d02c7e14af6ull, 0xc480f0cf064dd592ull, 0x3eb0c6f7a0b5ed8dull};
    long nfmt = 0;
    for (uint64_t b : fbits) {
        double d;
        memcpy(&d, &b, 8);
        for (int cap : {0, 1, 5, 30, 31, 400}) {
            std::vector<char> buf((size_t) (cap ? cap : 1));
            if (flbgpu_nc_fmt_f6(d, buf.data(), cap) > cap) return 3;
            nfmt++;
        }
    }
    const long long ints[] = {0, 1, -1, 9, 10, -10, 1ll << 32, (1ll << 53) + 1, INT64_MAX, INT64_MIN, INT64_MIN + 1, -42};
    for (long long v : ints) {
        char buf[20];                                                    // "%ld" writes at most 20 characters
        if (flbgpu_nc_fmt_ld(v, buf) > 20) return 3;
        nfmt++;
    }
    printf("numbers: %ld formats\nclean\n", nfmt);
    return 0;
}
