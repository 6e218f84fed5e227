// mlfilter.hpp -- filter_multiline's host side (mlfilter.cpp) and what it reads of the multiline core (ml.cpp)
#pragma once
#include "host_int.hpp"

namespace flbgpu {
bool ml_parser_args(const flbgpu_ml_parser *p, MlArgs &a, std::string &key_content, bool &has_sub, int &nrules);
constexpr int MLF_TRUNC_ROUNDS = 4096;          // truncating continuations settled per call, as flbgpu_ml_append_dev's ML_TRUNC_ROUNDS

// what one stream carries from call to call (buffer off: ONE stream per instance, and its buffers are empty between calls -- buffered
// mode will keep one of these per (input, tag), next to a carried first-line map)
struct MlfStream {
    uint32_t state = 0;                         // rule_to_state: 0 none, r + 1
    uint32_t sec = 0, nsec = 0;                 // flb_ml_stream_group.mp_time: the time registered last
};
// flbgpu_multiline_counters
struct MlfTotals { uint64_t ok_records = 0, truncations = 0, handed_back = 0, mismatch = 0; };

// ---- the host side of a call's bookkeeping (run_mlfilter_dev), free of device calls so that it can be driven with made-up words
// the rows of the call: all of them, or the rows in front of the first one the decoder refuses (0: nothing to do)
uint64_t mlf_rows_of_call(uint64_t n, unsigned long long first_bad);
// after a scan round: MLF_ROUND_DONE no truncating continuation is left, MLF_ROUND_AGAIN pin trunc_k and scan again, MLF_ROUND_OVER
// the call has used up its rounds and fails
enum { MLF_ROUND_DONE = 0, MLF_ROUND_AGAIN = 1, MLF_ROUND_OVER = 2 };
int mlf_round_step(uint64_t round, uint64_t items, unsigned long long trunc_k);
// what the call's words say: MLF_GO, MLF_HAND_BACK (the call answers -1 and is counted; `why` says which record), MLF_FAIL (no output;
// a mismatch is counted).  The stream is never touched here.
enum { MLF_GO = 0, MLF_HAND_BACK = 1, MLF_FAIL = 2 };
int mlf_judge(const MlfWords &w, MlfTotals &t, std::string &why);
// a call that succeeded: the stream moves, the totals grow
void mlf_commit(MlfStream &s, MlfTotals &t, bool regex, uint32_t final_state, const MlfWords &w, uint64_t kept);
}
