// multiline_filter_sanitize.cpp -- a stand-alone driver for the host code of filter_multiline under AddressSanitizer and
// UndefinedBehaviorSanitizer.  It needs no device.
//   * the front end: flbgpu_multiline_parse_check and flbgpu_filter_multiline_create (csrc/mlfilter.cpp) over accepted and refused
//     configurations -- property names without case, lists of parser names with blanks and empty entries, long names, missing
//     handles.  Without a device create refuses every configuration that reaches the parser (the built-ins' tables live on the device):
//     every object built on the way is freed again.
//   * the host side of a call's bookkeeping, which MlFilterState::run keeps in functions free of device calls (csrc/mlfilter.hpp), driven
//     with made-up device words: the rows in front of a decoder error, the truncation rounds up to their limit, what the words of a call
//     mean (go on / hand back and count / fail), and the stream and the totals moving on success only.
// mlfilter.cpp and the filters' shared front (filter_host.cpp) are compiled into the program with the sanitizers; what they call
// outside themselves comes from the ordinary libflbgpu.so:
//
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -O1 -g -std=c++17 \
//       -o multiline_filter_sanitize tools/multiline_filter_sanitize.cpp fluent-bit_amd/csrc/mlfilter.cpp fluent-bit_amd/csrc/filter_host.cpp \
//       -Lfluent-bit_amd/csrc -lflbgpu -Wl,-rpath,$PWD/fluent-bit_amd/csrc
//   ./multiline_filter_sanitize
//
// It prints how many configurations were accepted and refused and how many bookkeeping checks ran, and ends with "clean" and status
// 0; a failed check or a sanitizer report ends it with another status.
#include "../fluent-bit_amd/csrc/mlfilter.hpp"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

typedef std::vector<std::pair<std::string, std::string>> Props;

// the call's bookkeeping with made-up words; returns the number of checks, or minus the number of the one that failed
static int bookkeeping() {
    using namespace flbgpu;
    int n = 0;
#define CHECK(x) do { n++; if (!(x)) return -n; } while (0)
    // the rows of the call
    CHECK(mlf_rows_of_call(10, ~0ull) == 10);
    CHECK(mlf_rows_of_call(10, 0) == 0);
    CHECK(mlf_rows_of_call(10, 7) == 7);
    CHECK(mlf_rows_of_call(10, 99) == 10);
    CHECK(mlf_rows_of_call(0, ~0ull) == 0);
    // the truncation rounds: every round pins the item the device named, until none is left or the rounds are used up
    CHECK(mlf_round_step(0, 5, ~0ull) == MLF_ROUND_DONE);
    CHECK(mlf_round_step(0, 5, 3) == MLF_ROUND_AGAIN);
    CHECK(mlf_round_step(5, 5, 3) == MLF_ROUND_AGAIN);
    CHECK(mlf_round_step(6, 5, 3) == MLF_ROUND_OVER);
    CHECK(mlf_round_step(0, 5, 5) == MLF_ROUND_OVER);                 // an item that is not there is never pinned
    CHECK(mlf_round_step(MLF_TRUNC_ROUNDS - 1, 1u << 20, 9) == MLF_ROUND_AGAIN);
    CHECK(mlf_round_step(MLF_TRUNC_ROUNDS, 1u << 20, 9) == MLF_ROUND_OVER);
    CHECK(mlf_round_step(~0ull, ~0ull, ~0ull - 1) == MLF_ROUND_OVER);
    uint64_t rounds = 0;
    for (uint64_t k = 1; mlf_round_step(rounds, 1u << 20, k) == MLF_ROUND_AGAIN; k++) rounds++;
    CHECK(rounds == (uint64_t) MLF_TRUNC_ROUNDS);
    // what the words mean; the stream is not theirs to touch
    MlfStream s;
    s.state = 3; s.sec = 11; s.nsec = 12;
    MlfTotals t;
    std::string why;
    MlfWords w;
    memset(&w, 0, sizeof(w));
    CHECK(mlf_judge(w, t, why) == MLF_GO && t.handed_back == 0 && t.mismatch == 0);
    w.meta_refused = 2;
    CHECK(mlf_judge(w, t, why) == MLF_HAND_BACK && t.handed_back == 1 && why.find("metadata") != std::string::npos);
    w.meta_refused = 0; w.empty_start = ~0ull;
    CHECK(mlf_judge(w, t, why) == MLF_HAND_BACK && t.handed_back == 2 && why.find("empty text") != std::string::npos);
    w.big = 1;                                                        // (a size that does not fit comes before everything the sizes depend on)
    CHECK(mlf_judge(w, t, why) == MLF_FAIL && t.handed_back == 2);
    w.big = 0; w.empty_start = 0; w.mismatch = 5;
    CHECK(mlf_judge(w, t, why) == MLF_FAIL && t.mismatch == 5 && t.handed_back == 2);
    w.mismatch = ~0ull;
    CHECK(mlf_judge(w, t, why) == MLF_FAIL && t.mismatch == 4);       // (wraps like the device's own counter would)
    CHECK(s.state == 3 && s.sec == 11 && s.nsec == 12 && t.ok_records == 0 && t.truncations == 0);
    // a call that succeeded
    memset(&w, 0, sizeof(w));
    w.truncated = 3; w.has_reg = 1; w.last_sec = 100; w.last_nsec = 200;
    mlf_commit(s, t, true, 7, w, 10);
    CHECK(s.state == 7 && s.sec == 100 && s.nsec == 200 && t.ok_records == 7 && t.truncations == 3);
    w.has_reg = 0; w.truncated = 0; w.last_sec = 1; w.last_nsec = 1;
    mlf_commit(s, t, false, 9, w, 4);                                 // ENDSWITH / EQ keep no rule state; no registration: the time stays
    CHECK(s.state == 7 && s.sec == 100 && s.nsec == 200 && t.ok_records == 11 && t.truncations == 3);
    w.truncated = 99;
    mlf_commit(s, t, true, 0, w, 4);                                  // more truncations than records cannot be: nothing goes below zero
    CHECK(s.state == 0 && t.ok_records == 11 && t.truncations == 7);
#undef CHECK
    return n;
}

int main() {
    const std::vector<std::string> pnames = {"mine", "", "other", std::string(300, 'p')};
    std::vector<const char *> pn;
    for (const auto &s : pnames) pn.push_back(s.c_str());
    std::vector<flbgpu_ml_parser *> ph(pnames.size(), nullptr);
    const std::vector<std::string> parsers = {"java", "go", "python", "ruby", "mine", " mine ", "mine,", ",,mine", "mine, java", "docker", "cri", "nope", "", " ", ",",
                                              std::string(300, 'p'), std::string(5000, ','), "Java"};
    const std::vector<std::string> buffers = {"off", "OFF", "false", "no", "on", "true", "0", "1", "", "offf"};
    const std::vector<std::string> modes = {"", "parser", "PARSER", "partial_message", "Partial_Message", "x"};
    const std::vector<std::string> keys = {"", "log", std::string(255, 'k'), std::string(256, 'k'), std::string("a\tb")};
    int accepted = 0, refused = 0, created = 0;
    for (const auto &p : parsers) for (const auto &b : buffers) for (const auto &m : modes) for (const auto &k : keys) {
        Props pr = {{"Multiline.Parser", p}, {"BUFFER", b}, {"flush_ms", "100"}, {"emitter_name", "e"}, {"debug_flush", "x"}};
        if (!m.empty()) pr.push_back({"mode", m});
        if (!k.empty()) pr.push_back({"multiline.key_content", k});
        if (k.size() == 3 && b == "off") pr.push_back({"unknown.name", "1"});
        std::vector<const char *> n, v;
        for (const auto &kv : pr) { n.push_back(kv.first.c_str()); v.push_back(kv.second.c_str()); }
        for (size_t cap : {(size_t) 0, (size_t) 1, (size_t) 16, (size_t) 4096}) {
            std::vector<char> desc(cap ? cap : 1);
            const int r = flbgpu_multiline_parse_check((int) pr.size(), n.data(), v.data(), (int) pn.size(), pn.data(), ph.data(), cap ? desc.data() : nullptr, cap);
            if (cap == 4096) { if (r == 0) accepted++; else refused++; }
        }
        // without a device every create ends in a refusal -- after the configuration was parsed and, for a built-in, after the parser was asked for
        flbgpu_filter *f = flbgpu_filter_multiline_create((int) pr.size(), n.data(), v.data(), (int) pn.size(), pn.data(), ph.data());
        if (f) { uint64_t c[4]; flbgpu_multiline_counters(f, c); (void) flbgpu_multiline_state(f); flbgpu_filter_destroy(f); created++; }
    }
    // arguments that are not there
    const char *one[1] = {"buffer"}, *none[1] = {nullptr};
    if (flbgpu_multiline_parse_check(1, one, none, 0, nullptr, nullptr, nullptr, 0) == 0) return 1;
    if (flbgpu_multiline_parse_check(-1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0) == 0) return 1;
    if (flbgpu_multiline_parse_check(0, nullptr, nullptr, 3, nullptr, nullptr, nullptr, 0) == 0) return 1;
    uint64_t c[4];
    flbgpu_multiline_counters(nullptr, c);
    if (flbgpu_multiline_state(nullptr) != -1) return 1;
    printf("configurations: %d accepted, %d refused; %d filters created\n", accepted, refused, created);
    if (accepted == 0 || refused == 0) return 1;
    const int checks = bookkeeping();
    if (checks < 0) { printf("bookkeeping check %d failed\n", -checks); return 1; }
    printf("bookkeeping: %d checks\n", checks);
    printf("clean\n");
    return 0;
}
