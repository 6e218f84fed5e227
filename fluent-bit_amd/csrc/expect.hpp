// expect.hpp -- filter_expect's program as the device sees it (expect.cpp builds it, expect_kernels.inc runs it)
// plugins/filter_expect/expect.c:146-230 (context_create, behind the config map of :580-632), 275-396 (rule_apply), 398-564 (one call)
//
// Limits and refusals at create time (DESIGN 8 lists them): a property set twice that the config map takes once (action, result_key),
// an unknown property, an unknown action, an accessor the record accessor's grammar refuses, a key_val_eq without a value (the
// reference takes the first and the last entry of an empty list), `${` in a value, more than EX_MAX_RULES rules, a table over
// TC_MAX_TABLE_BYTES, a result_key over 65535 bytes.
#pragma once
#include <cstdint>
#include "dev.hpp"
#include "typeconv.hpp"

namespace flbgpu {

constexpr int EX_MAX_RULES = 64;
constexpr uint32_t EX_MAX_RESULT_KEY = 65535;
constexpr int EX_BLOCK = 256;

enum { EX_WARN = 0, EX_EXIT = 1, EX_RESULT_KEY = 2 };
// rule kinds; EX_ACTION is the rule an `action` property leaves in the list (type -1 in the reference): it passes always and takes a number
enum { EX_KEY_EXISTS = 0, EX_KEY_NOT_EXISTS = 1, EX_KEY_VAL_NULL = 2, EX_KEY_VAL_NOT_NULL = 3, EX_KEY_VAL_EQ = 4, EX_ACTION = 5 };
// how a rule failed
enum { EXF_NOT_FOUND = 1, EXF_EXISTS = 2, EXF_WRONG_TYPE = 3, EXF_DIFFERENT = 4 };
// the value the rule met, as msgpack_object_to_ra_value types it (src/flb_ra_key.c:31-105); an ARRAY or EXT is not found at all
enum { EXT_NONE = 0, EXT_BOOL = 1, EXT_INT = 2, EXT_FLOAT = 3, EXT_STRING = 4, EXT_NULL = 5, EXT_BINARY = 6 };
// the passes of k_expect
enum { EX_CHECK = 0, EX_SIZE = 1, EX_EMIT = 2 };

// the verdict word of a row: bits 0-7 the failing rule's number, 8-11 how it failed, 12-15 the value's type
constexpr uint32_t EXV_FAILED = 1u << 16;          // a rule failed
constexpr uint32_t EXV_CHECKED = 1u << 17;         // the decoder handed the row on as a record and the rules ran
constexpr uint32_t EXV_RAW = 1u << 18;             // a group marker: goes out as its own bytes under result_key

// the table in LDS (words):
//   [0] number of rules    [1] action    [2] bytes of the packed result key (STR header and name)    [3] their byte offset
//   then per rule eight words: { kind, accessor: length of the key name | number of sub-keys << 16 | EX_ACC_INERT, byte offset of the
//   key name, byte offset of the sub-key list (ra_lds.inc's two words per sub-key), length of the expected text, its byte offset, 0, 0 },
//   then the sub-key lists and the bytes, each padded to a multiple of 4
constexpr uint32_t EX_HDR_WORDS = 4, EX_RULE_WORDS = 8;
constexpr uint32_t EX_ACC_INERT = 1u << 31;

// one entry of the failure table (the C ABI's flbgpu_expect_failure)
struct ExFailure {
    uint64_t in_off, val_off;       // the record and -- for a STR value -- its payload, as offsets into the input chunk
    uint32_t len, val_len;
    uint32_t rule, kind, vtype, reserved;
};

struct ExpectArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;      // HBM copy of the LDS table
    uint32_t table_bytes;
    uint32_t *verdict;          // [n]
    uint32_t *val_off, *val_len;    // [n] a STR value's payload, relative to the row
    uint32_t *fail;             // [n] 1 where a rule failed (the failure table's scan runs over it)
    uint32_t *len;              // [n] size pass: output bytes of the row
    // [0] first row the decoder refuses, [1] first row a rule failed on
    unsigned long long *firsts;
    // [0] records checked, [1] records failed, [2] records emitted, [3] rows over 4 GB, [4] rows whose emitted length differs from
    // their sized length
    unsigned long long *counts;
    const uint64_t *out_off;
    uint8_t *out;
    const uint64_t *fail_idx;   // [n + 1] the scan over fail[]
    ExFailure *fail_tbl;
    uint64_t fail_cap;
};

void launch_expect(const ExpectArgs &a, int pass, hipStream_t st);
void launch_expect_table(const ExpectArgs &a, hipStream_t st);

}  // namespace flbgpu
