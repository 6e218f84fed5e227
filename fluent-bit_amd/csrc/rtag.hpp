// rtag.hpp -- filter_rewrite_tag's program as the device sees it (rtag.cpp builds it, rtag_kernels.inc runs it)
// plugins/filter_rewrite_tag/rewrite_tag.c:112-190 (process_config), 356-423 (process_record), 425-557 (one call), 590-613 (config map);
// src/flb_record_accessor.c:74-230 (the parts of an accessor), 456-619 (ra_translate_*), 644-699 (flb_ra_translate_check), 753-764
// (flb_ra_regex_match); src/flb_ra_key.c:31- (msgpack_object_to_ra_value), 108-135 (ra_key_val_id), 374- (flb_ra_key_regex_match)
//
// Limits, refused at create time (the reference has none of them):
//   * more than RT_MAX_RULES rules, a template of more than RT_MAX_PARTS parts, a rule table of more than RT_MAX_TABLE_BYTES bytes;
//   * a key name of MAX_KEY bytes or more, more than MAX_SUBKEYS sub-keys or more than 256 bytes of sub-key names in one `$key...`;
//   * a `$key...` whose name does not start with a letter or '_';
//   * `$n` with n > 9 in NEW_TAG where the pattern has a group n (atoi reads `$12` as group 12; a captured row keeps the spans of groups
//     0 .. 9; without such a group the part adds nothing, as with the reference), and a pattern with more than RT_MAX_GROUPS capture
//     groups next to a NEW_TAG that holds a `$n`;
//   * a pattern that is not a regular expression (look-around, back-references, atomic groups ...): the emitted tag needs the match
//     on the device, and the host's backtracking matcher is not wired into this filter.
#pragma once
#include <cstdint>
#include "dev.hpp"

namespace flbgpu {

constexpr int RT_MAX_RULES = 32;
constexpr int RT_MAX_PARTS = 16;                   // parts of one NEW_TAG
constexpr uint32_t RT_MAX_TABLE_BYTES = 24576;     // the whole table (it sits in LDS)
constexpr int RT_MAX_GROUPS = 31;                  // capture groups of a pattern whose template reads one (slot2cap has 2 * MAX_GROUPS entries)
constexpr int RT_BLOCK = 256;
constexpr uint32_t RT_CAP_COLS = 20;               // span columns of a captured row: begin / end of groups 0 .. 9

// what the match pass writes per row
constexpr uint32_t RT_ROW_NONE = 0xFFFFFFFFu;      // a record no rule matched
constexpr uint32_t RT_ROW_SKIP = 0xFFFFFFFEu;      // a row the decoder does not hand out (a group marker, a record an earlier filter dropped)

constexpr uint32_t RT_RULE_WORDS = 6, RT_PART_WORDS = 4;
constexpr uint32_t RT_KEEP = 1u, RT_INERT = 2u, RT_NEEDS_CAP = 4u;
enum { RT_P_STR = 0, RT_P_TAG = 1, RT_P_TAGPART = 2, RT_P_REGEX = 3, RT_P_KEY = 4 };     // = RA_* of host_int.hpp

// the table: RT_RULE_WORDS words per rule
//   [0] RT_KEEP | RT_INERT (KEY's first part has no key: the rule never matches) | RT_NEEDS_CAP | sub-keys of KEY << 8 | parts of NEW_TAG << 16
//   [1] length of KEY's name            [2] its byte offset inside the table
//   [3] byte offset of KEY's sub-key list (ra_lds.inc)
//   [4] byte offset of the part list: RT_PART_WORDS words per part
//         [0] kind | sub-keys << 8      [1] STR: length of the text, KEY: length of the name, TAGPART / REGEX: the id (as int32)
//         [2] byte offset of the text / name        [3] byte offset of the sub-key list
//   [5] index of the rule's capture program in RtagArgs::caps (RT_NEEDS_CAP)
// then the lists and the bytes, each entry padded to a multiple of 4

// a rule's capture program (compiled only where NEW_TAG holds a `$n`): both table sets and the NUMBER -> column map
struct RtagCap {
    DevCap ascii, utf8;
    uint8_t slot2cap[2 * MAX_GROUPS];   // capture slot 2g / 2g + 1 -> span column 2g / 2g + 1 for g <= 9, 0xFF otherwise
    int ngroups;                        // what flb_regex_do answers (num_regs - 1): 0 leaves the result without a region, `$0` adds nothing
};

struct RtagEmitted {                    // = flbgpu_rtag_emitted_rec (include/flb_gpu.h)
    uint64_t in_off, tag_off;
    uint32_t len, tag_len;
};

struct RtagArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;      // HBM copy of the table; every workgroup loads it into LDS
    uint32_t table_bytes;
    int nrules;
    const GrepRule *rules;      // [nrules] match-only DFA + UTF-8 tables (key unused)
    const RtagCap *caps;        // capture programs
    const uint8_t *tag;         // the call's tag
    uint32_t tag_len;
    uint32_t *rule;             // [n] the rule that matched the row, RT_ROW_NONE, RT_ROW_SKIP
    uint32_t *keep_len;         // [n] bytes of the row in the output (its length or 0)
    uint32_t *emit;             // [n] 1: the row is emitted
    const uint64_t *emit_idx;   // [n + 1] exclusive scan of emit
    uint32_t *tag_lens;         // [n] bytes of the row's tag (size pass)
    const uint64_t *tag_off;    // [n + 1] exclusive scan of tag_lens (emit pass)
    uint8_t *tags;              // the tag arena
    RtagEmitted *table_out;     // [emitted rows]
    uint32_t *spans;            // [RT_CAP_COLS][n_emit] capture spans of the emitted rows (size pass writes, emit pass reads)
    uint64_t n_emit;
    uint16_t *chk;              // the capture walk's scratch: [waves][chk_len][64]
    uint32_t chk_len, chk_nfa_off;
    unsigned long long *first_bad;    // first row the decoder refuses
    // [0] decoded records, [1] kept records, [2] matched records, [3] rows whose emitted span does not fit 32 bits,
    // [4] rows whose tag was written with another length than it was sized with, or whose capture walk failed, [5] tag bytes
    unsigned long long *counts;
};

void launch_rtag_match(const RtagArgs &a, hipStream_t st);
void launch_rtag(const RtagArgs &a, bool emit, int waves, hipStream_t st);
// a refused emission keeps its record: keep_len[row] = the row's length for the emitted rows whose bit is set in `refused`
void launch_rtag_refuse(const RtagArgs &a, const uint32_t *refused, hipStream_t st);

}  // namespace flbgpu
