// nest.hpp -- filter_nest's program as the device sees it (nest.cpp builds it, nest_kernels.inc runs it)
// plugins/filter_nest/nest.c:57-175 (configure), 298-345 (is_kv_to_nest), 353-397 (is_kv_to_lift), 473-606 (the rules), 631-717 (one call)
#pragma once
#include <cstdint>
#include "dev.hpp"

namespace flbgpu {

constexpr int NEST_MAX_WILDCARDS = 64;
constexpr uint32_t NEST_MAX_KEY_BYTES = 32768;      // the wildcards, the key and the prefix together (the table sits in LDS)
constexpr int NEST_BLOCK = 256;
constexpr uint32_t NEST_PREFIX = 0x80000000u;       // flag in a wildcard's length word: a trailing '*' was cut off (key_is_dynamic)

enum { NEST_OP_NEST = 1, NEST_OP_LIFT = 2 };
enum { NEST_PFX_NONE = 0, NEST_PFX_ADD = 1, NEST_PFX_REMOVE = 2 };
enum { NEST_ROW_NONE = 0, NEST_ROW_RAW = 1, NEST_ROW_BUILT = 2 };

// the table: 2 * nwild words { length | NEST_PREFIX, byte offset of the entry inside the table (a multiple of 4) }, then the
// wildcards' bytes, the key's and the prefix's, each padded to a multiple of 4
struct NestArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;      // HBM copy of the table; every workgroup loads it into LDS
    uint32_t table_bytes;
    int op;                     // NEST_OP_NEST / NEST_OP_LIFT
    int nwild;
    int has_key;                // Nest_under / Nested_under was given (a nest without it loses every record it would change)
    uint32_t key_off, key_len;  // the key inside the table
    int pfx;                    // NEST_PFX_*
    uint32_t pfx_off, pfx_len;  // the prefix inside the table
    uint32_t *len;              // [n] output bytes of the row (0: nothing is emitted for it)
    uint8_t *mode;              // [n] NEST_ROW_*: the row goes out as its own bytes or is built again
    unsigned long long *first_bad;    // first row the decoder refuses
    // [0] decoded records, [1] emitted records, [2] records built again, [3] rows over 4 GB, [4] compares that would have read past
    // the record, [5] records the reference leaves undefined
    unsigned long long *counts;
    const uint64_t *out_off;    // emit pass: [n + 1] exclusive scan of len
    uint8_t *out;
};

void launch_nest(const NestArgs &a, bool emit, hipStream_t st);

}  // namespace flbgpu
