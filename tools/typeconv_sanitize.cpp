// typeconv_sanitize.cpp -- a stand-alone driver for the host code of filter_type_converter under AddressSanitizer and
// UndefinedBehaviorSanitizer: flbgpu_type_converter_parse_check (csrc/typeconv.cpp) over the front-end cases and the flbgpu_nc_*
// functions filter_type_converter added (csrc/numconv_host.cpp) over the number edges.  It needs no device.  typeconv.cpp, the
// filters' shared front (filter_host.cpp) and numconv_host.cpp are compiled into the program with the sanitizers; what they call outside themselves (the record accessor's
// parser, the token splitter) comes from the ordinary libflbgpu.so:
//
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -O1 -g -std=c++17 \
//       -o typeconv_sanitize tools/typeconv_sanitize.cpp fluent-bit_amd/csrc/typeconv.cpp fluent-bit_amd/csrc/filter_host.cpp \
//       fluent-bit_amd/csrc/numconv_host.cpp -Lfluent-bit_amd/csrc -lflbgpu -Wl,-rpath,$PWD/fluent-bit_amd/csrc
//   ./typeconv_sanitize
//
// It prints how many programs were accepted and refused and how many numbers went through, and ends with "clean" and status 0; a
// sanitizer report ends it with another status.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

extern "C" {
int flbgpu_type_converter_parse_check(int nprops, const char *const *names, const char *const *values, char *desc, size_t cap);
unsigned long long flbgpu_nc_scan_intmax(const char *s, int len, int base, int is_signed);
int flbgpu_nc_fmt_lu(unsigned long long v, char *buf);
double flbgpu_nc_int_to_double(unsigned long long v, int is_signed);
unsigned long long flbgpu_nc_double_to_int(double v, int is_signed, int *undef);
int flbgpu_nc_fmt_json_double(double v, int nan_to_null, char *buf);
int flbgpu_nc_scan_double(const char *s, int len, int mode, int exact, double *out, int *consumed);
}

typedef std::vector<std::pair<std::string, std::string>> Props;

static int check(const Props &p, size_t cap) {
    std::vector<const char *> n, v;
    for (const auto &kv : p) { n.push_back(kv.first.c_str()); v.push_back(kv.second.c_str()); }
    std::vector<char> desc(cap ? cap : 1);
    return flbgpu_type_converter_parse_check((int) p.size(), n.data(), v.data(), cap ? desc.data() : nullptr, cap);
}

int main() {
    std::vector<Props> progs = {
        {{"str_key", "a b int"}}, {{"STR_KEY", "a b i"}, {"Int_Key", "c d s"}, {"uint_key", "e f f"}, {"float_key", "g h u"}},
        {{"str_key", "a b int extra words"}, {"int_key", "c d string"}}, {{"str_key", "a b int extra"}}, {{"str_key", "a b"}}, {{"str_key", "a"}},
        {{"str_key", ""}}, {{"str_key", "   "}}, {}, {{"bool_key", "a b string"}}, {{"", ""}}, {{"str_key", "a b integer"}}, {{"str_key", "a b strings"}},
        {{"str_key", "a b \"\""}}, {{"str_key", "\"a b\" \"c d\" int"}}, {{"str_key", "\"a b c"}}, {{"str_key", "a \"b\\\" c\" int"}}, {{"str_key", "a b \""}},
        {{"str_key", "$a b int"}}, {{"str_key", "$a['b']['c'] t int"}}, {{"str_key", "$a['l'][3] t int"}}, {{"str_key", "$a[0][1] t int"}},
        {{"str_key", "$a['it''s'] t int"}}, {{"str_key", "$a['x.y'] t int"}}, {{"str_key", "pre$key t int"}}, {{"str_key", "pre$key['a t int"}},
        {{"str_key", "$TAG t int"}}, {{"str_key", "$TAG[2] t int"}}, {{"str_key", "$TAG[ t int"}}, {{"str_key", "$TAG[] t int"}}, {{"str_key", "$TAGS t int"}},
        {{"str_key", "$TA t int"}}, {{"str_key", "$0 t int"}}, {{"str_key", "$9x t int"}}, {{"str_key", "$ t int"}}, {{"str_key", "$$ t int"}},
        {{"str_key", "$a.b t int"}}, {{"str_key", "$a.b['c t int"}}, {{"str_key", "a.b t int"}}, {{"str_key", "a$ t int"}}, {{"str_key", "x t int"}},
        {{"str_key", "$a$b t int"}}, {{"str_key", "$a,b t int"}}, {{"str_key", "$a['x t int"}}, {{"str_key", "$a[x] t int"}}, {{"str_key", "$a['x']y t int"}},
        {{"str_key", "$a[1 t int"}}, {{"str_key", "$a[ t int"}}, {{"str_key", "$a[' t int"}}, {{"str_key", "$-a t int"}}, {{"str_key", "$a[99999999999999999999] t int"}},
        {{"str_key", "$" + std::string(127, 'k') + " t int"}}, {{"str_key", "$" + std::string(128, 'k') + " t int"}},
        {{"str_key", std::string(127, 'k') + " t int"}}, {{"str_key", std::string(128, 'k') + " t int"}}, {{"str_key", std::string(5000, 'k') + "$a t int"}},
        {{"str_key", "$a['" + std::string(256, 's') + "'] t int"}}, {{"str_key", "$a['" + std::string(257, 's') + "'] t int"}},
        {{"str_key", "abcd " + std::string(32768 - 24 - 4 - 3, 't') + " int"}}, {{"str_key", "abcd " + std::string(32769 - 24 - 4 - 3, 't') + " int"}},
        {{"str_key", "a " + std::string(70000, 't') + " int"}}, {{"str_key", "a b " + std::string(70000, 'i')}},
    };
    {
        std::string subs8, subs9;
        for (int i = 0; i < 9; i++) { if (i < 8) subs8 += "['s']"; subs9 += "['s']"; }
        progs.push_back({{"str_key", "$a" + subs8 + " t int"}});
        progs.push_back({{"str_key", "$a" + subs9 + " t int"}});
        Props p64, p65, skipped;
        for (int i = 0; i < 65; i++) {
            const std::string r = "k" + std::to_string(i) + " t" + std::to_string(i) + " int";
            if (i < 64) p64.push_back({"str_key", r});
            p65.push_back({"str_key", r});
            skipped.push_back({"str_key", r + " extra"});
        }
        skipped.push_back({"str_key", "a b int"});
        progs.push_back(p64); progs.push_back(p65); progs.push_back(skipped);
    }
    int ok = 0, refused = 0;
    for (const Props &p : progs)
        for (size_t cap : {(size_t) 0, (size_t) 1, (size_t) 2, (size_t) 17, (size_t) 1 << 17}) { if (check(p, cap) == 0) ok++; else refused++; }
    if (flbgpu_type_converter_parse_check(-1, nullptr, nullptr, nullptr, 0) == 0 || flbgpu_type_converter_parse_check(1, nullptr, nullptr, nullptr, 0) == 0) return 2;
    { const char *n[1] = {nullptr}, *v[1] = {nullptr}; if (flbgpu_type_converter_parse_check(1, n, v, nullptr, 0) == 0) return 2; }
    printf("front end: %d answers accepted, %d refused\n", ok, refused);

    // ---- numbers: every text in a buffer of exactly its length, so that a read past it is a report
    const std::vector<std::string> texts = {
        "", " ", "0", "-0", "  -0", "7", "\t7", "\n7", "\v7", "\f7", "\r7", "-", "+", "-+1", "12abc", "abc", "0x", "0X", "0xg", "0x1f", "-0x1f", "+0x",
        "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "18446744073709551615", "18446744073709551616",
        "-18446744073709551615", "123456789012345678901234567890", "ffffffffffffffff", "0x10000000000000001", std::string("1\0002", 3), std::string("\0001", 2),
        std::string(40, '0') + "5", "nan", "-nan", "nan()", "nan(0x12)", "nan(0x12", "nan(abc)", "nan(0777)", "nan(99999999999999999999)", "NAN(1)x", "inf",
        "-infinity", "1.5", "1e400", "4.9e-324", "0x1.8p1", "2.2250738585072011e-308", ".", "1e", std::string(3000, '9'), "0." + std::string(1200, '0') + "1"};
    long nscan = 0;
    for (const std::string &t : texts) {
        std::vector<char> exact(t.begin(), t.end());
        for (int len = 0; len <= (int) exact.size(); len++) {
            if (exact.size() > 64 && len != (int) exact.size()) continue;
            std::vector<char> cut(exact.begin(), exact.begin() + len);
            for (int base : {10, 16}) for (int sg : {0, 1}) { flbgpu_nc_scan_intmax(cut.data(), len, base, sg); nscan++; }
            double d; int used;
            for (int mode : {0, 1, 0x100, 0x101}) { flbgpu_nc_scan_double(cut.data(), len, mode, 1, &d, &used); nscan++; }
        }
    }
    const uint64_t ints[] = {0, 1, 9, 10, 1ull << 32, (1ull << 53) + 1, (1ull << 63) - 1, 1ull << 63, ~0ull, ~0ull - 1024, 9007199254740993ull};
    const uint64_t fbits[] = {0, 0x8000000000000000ull, 0x3ff0000000000000ull, 0xbff8000000000000ull, 0x43e0000000000000ull, 0xc3e0000000000000ull,
                              0x43dfffffffffffffull, 0x43f0000000000000ull, 0x7ff0000000000000ull, 0xfff0000000000000ull, 0x7ff8000000000000ull,
                              0xfff8000000000123ull, 1, 0x7fefffffffffffffull, 0x444b1ae4d6e2ef50ull, 0x405edd2f1a9fbe77ull, 0x3fb999999999999aull,
                              0xc3e0000000000001ull, 0x7e37e43c8800759cull, 0xfe37e43c8800759cull};
    long nfmt = 0;
    for (uint64_t v : ints) {
        char buf[24];                                                    // "%lu" writes at most 20 characters
        flbgpu_nc_fmt_lu(v, buf);
        flbgpu_nc_int_to_double(v, 0); flbgpu_nc_int_to_double(v, 1);
        nfmt += 3;
    }
    for (uint64_t b : fbits) {
        double d; memcpy(&d, &b, 8);
        char buf[32];                                                    // "%.16g" / "%.1f" of an integral value below 2^63: at most 24
        int undef = 0;
        flbgpu_nc_fmt_json_double(d, 0, buf);
        flbgpu_nc_double_to_int(d, 0, &undef); flbgpu_nc_double_to_int(d, 1, &undef); flbgpu_nc_double_to_int(d, 1, nullptr);
        nfmt += 4;
    }
    printf("numbers: %ld scans, %ld casts and formats\nclean\n", nscan, nfmt);
    return 0;
}
