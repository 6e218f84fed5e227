// recmod.hpp -- filter_record_modifier's program as the device sees it (recmod.cpp builds it, recmod_kernels.inc runs it)
// plugins/filter_record_modifier/filter_modifier.c:69-155 (configure), 213-279 (make_bool_map), 298-486 (one call)
#pragma once
#include <cstdint>
#include "dev.hpp"

namespace flbgpu {

constexpr int RECMOD_MAX_RECORDS = 64, RECMOD_MAX_KEYS = 64;
constexpr uint32_t RECMOD_MAX_KEY_BYTES = 32768;    // all key entries together (the table sits in LDS)
constexpr int RECMOD_BLOCK = 256;
constexpr uint32_t RECMOD_PREFIX = 0x80000000u;     // flag in a table entry's length word: a trailing '*' was cut off (dynamic_key)

enum { RECMOD_NONE = 0, RECMOD_REMOVE = 1, RECMOD_ALLOW = 2 };

// the key table: 2 * nkeys words { length | RECMOD_PREFIX, byte offset of the entry inside the table (a multiple of 4) }, then the
// entries' bytes folded to lower case (ASCII only), each padded to a multiple of 4
struct RecmodArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;      // HBM copy of the key table; every workgroup loads it into LDS
    uint32_t table_bytes;
    int nkeys;
    int list;                   // RECMOD_NONE / RECMOD_REMOVE / RECMOD_ALLOW
    uint32_t nrec;              // Record entries
    const uint8_t *tail;        // the Record entries as msgpack (STR key, STR value, ...), encoded at create
    uint32_t tail_len;
    uint32_t *len;              // [n] output bytes of the row (0: nothing is emitted for it)
    unsigned long long *first_bad;    // first row the decoder refuses
    unsigned long long *first_wide;   // first row whose body has more than 65535 entries
    unsigned long long *counts; // [0] decoded records, [1] emitted records, [2] records that lost a key, [3] rows over 4 GB
    const uint64_t *out_off;    // emit pass: [n + 1] exclusive scan of len
    uint8_t *out;
};

void launch_recmod(const RecmodArgs &a, bool emit, hipStream_t st);

}  // namespace flbgpu
