// typeconv.hpp -- filter_type_converter's program as the device sees it (typeconv.cpp builds it, typeconv_kernels.inc runs it)
// plugins/filter_type_converter/type_converter.c:57-140 (config_rule, configure), 182-353 (one call); src/flb_typecast.c:27-49 (the
// type words), 72-341 (the conversions), 396-457 (the source-type checks)
//
// Limits, refused at create time (the reference has none of them):
//   * more than TC_MAX_RULES rules that configure() keeps, or a table of more than TC_MAX_TABLE_BYTES bytes;
//   * a from_key whose name is MAX_KEY bytes or longer, with more than MAX_SUBKEYS sub-keys, or whose sub-key names hold more
//     than 256 bytes together;
//   * a from_key `$x...` whose name does not start with a letter or '_' (the reference's lexer would have to be restated for it);
//   * a type word the type table does not know, and a from_key the accessor's grammar refuses (an open quote, `[x]`, bytes behind
//     the last `]`): config_rule frees such a rule with delete_conv_entry, which unlinks an entry that was never linked
//     (type_converter.c:52, 95-100), and the reference dies.
// Reproduced, not refused: `pre$key` looks up the key `pre` (the first part of the accessor decides, and it is the text in front
// of the '$'); `$TAG`, `$TAG[n]`, `$0`..`$9` and `$` alone make a rule that never finds its key; `$a.b` looks up `a` (the accessor
// ends at the '.').
#pragma once
#include <cstdint>
#include "dev.hpp"

namespace flbgpu {

constexpr int TC_MAX_RULES = 64;
constexpr uint32_t TC_MAX_TABLE_BYTES = 32768;     // the whole table (it sits in LDS)
constexpr int TC_BLOCK = 256;

enum { TC_SRC_STR = 0, TC_SRC_INT = 1, TC_SRC_UINT = 2, TC_SRC_FLOAT = 3 };
// flb_typecast_type_t in the order flb_typecast_str_to_type_t tries the words
enum { TC_TO_INT = 0, TC_TO_UINT = 1, TC_TO_FLOAT = 2, TC_TO_HEX = 3, TC_TO_STR = 4, TC_TO_BOOL = 5 };

constexpr uint32_t TC_RULE_WORDS = 6;
constexpr uint32_t TC_INERT = 1u << 24;            // flag in word 0: the accessor has no key part, the rule never finds anything
constexpr uint32_t TC_SUB_INDEX = 0x80000000u;     // flag in a sub-key's first word: an array index, not a name

// the table: TC_RULE_WORDS words per rule
//   [0] source class | target type << 8 | number of sub-keys << 16 | TC_INERT
//   [1] length of the key name          [2] its byte offset inside the table
//   [3] length of to_key as it goes out (a STR header and the bytes)   [4] its byte offset
//   [5] byte offset of the sub-key list: per sub-key two words { index | TC_SUB_INDEX, 0 } or { length, byte offset of the name }
// then the sub-key lists, then the bytes, each entry padded to a multiple of 4
struct TypeconvArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;      // HBM copy of the table; every workgroup loads it into LDS
    uint32_t table_bytes;
    int nrules;
    uint32_t *len;              // [n] output bytes of the row (0: nothing is emitted for it)
    unsigned long long *first_bad;    // first row the decoder refuses
    // [0] decoded records, [1] emitted records, [2] conversions done, [3] conversions failed, [4] conversions C leaves undefined,
    // [5] rows over 4 GB, [6] rows whose emitted length differs from their sized length (written by the emit pass)
    unsigned long long *counts;
    const uint64_t *out_off;    // emit pass: [n + 1] exclusive scan of len
    uint8_t *out;
};

void launch_typeconv(const TypeconvArgs &a, bool emit, hipStream_t st);

}  // namespace flbgpu
