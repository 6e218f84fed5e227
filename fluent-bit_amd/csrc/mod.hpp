// mod.hpp -- filter_modify's program as the device sees it (modify.cpp builds it, modify_kernels.inc runs it)
// plugins/filter_modify/modify.h:28-54 for the rule and condition types (their numbers are the reference's enum values)
#pragma once
#include <cstdint>
#include "dev.hpp"

namespace flbgpu {

constexpr int MOD_MAX_RULES = 64, MOD_MAX_CONDS = 32;
enum { MR_RENAME, MR_HARD_RENAME, MR_ADD, MR_SET, MR_REMOVE, MR_REMOVE_WILDCARD, MR_REMOVE_REGEX, MR_COPY, MR_HARD_COPY,
       MR_MOVE_TO_START, MR_MOVE_TO_END };
enum { MC_KEY_EXISTS, MC_KEY_DOES_NOT_EXIST, MC_A_KEY_MATCHES, MC_NO_KEY_MATCHES, MC_KEY_VALUE_EQUALS, MC_KEY_VALUE_DOES_NOT_EQUAL,
       MC_KEY_VALUE_MATCHES, MC_KEY_VALUE_DOES_NOT_MATCH, MC_MATCHING_KEYS_HAVE_MATCHING_VALUES,
       MC_MATCHING_KEYS_DO_NOT_HAVE_MATCHING_VALUES };

// strings live in one blob (ModArgs::str); a rule's key and value are string ids 2i and 2i + 1
struct ModRule {
    int type;
    uint32_t k_off, k_len, v_off, v_len;
    int rx;                     // Remove_regex: index into ModArgs::rx, else -1
};
struct ModCond {
    int type;
    int key;                    // index into ModArgs::keys; -1: an accessor whose first part is not a key (never finds a value)
    int rx_a, rx_b;             // executed patterns (index into ModArgs::rx), -1 when none
    uint32_t b_off, b_len;      // b as a string (b_len 0 when the condition has no b)
};

// the per-row entry list: u64 per entry -- bits 0..31 the original entry's key offset in the row (0xFFFFFFFF: none), 32..39 the
// string id of a key a rule wrote (0xFF: the original key), 40..47 the same for the value, 48 a rule's mark (modify_kernels.inc)
constexpr int MOD_LDS_ENTRIES = 32;             // entries per lane in LDS; a row that needs more takes its list from the arena in HBM
constexpr int MOD_BLOCK = 64;

struct ModArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const ModRule *rules;
    int nrules;
    const ModCond *conds;
    int nconds;
    const DevKey *keys;
    const GrepRule *rx;         // match-only DFA + UTF-8 tables of every executed pattern (only dfa / utf8 are used)
    const uint8_t *str;
    uint32_t true_off, false_off;
    int grow;                   // rules that can add an entry (Add, Set, Copy, Hard_copy)
    uint32_t *len;              // [n] output bytes of the row
    uint8_t *mod;               // [n] 1: the row is rebuilt, 0: copied as it is
    unsigned long long *first_bad;
    unsigned long long *counts; // [0] decoded records, [1] modified records, [2] prefix tests that ran past the record,
                                // [3] arena entries asked for, [4] rows whose arena slot did not fit
    unsigned long long *arena_top;
    uint64_t *arena;            // entry lists of rows that need more than MOD_LDS_ENTRIES
    uint64_t arena_cap;         // entries
    const uint64_t *out_off;    // emit pass: [n + 1] exclusive scan of len
    uint8_t *out;
};

void launch_modify(const ModArgs &a, bool emit, hipStream_t st);

}  // namespace flbgpu
