// checklist.hpp -- filter_checklist's program as the device sees it (checklist.cpp builds it, checklist_kernels.inc runs it)
// plugins/filter_checklist/checklist.c:130-196 (the list loader), 198-267 (init_config), 291-409 (set_record), 411-582 (one call)
//
// Limits and refusals at create time (DESIGN 8 lists them): a property the config map refuses, an unknown property, a lookup_key
// the accessor's grammar refuses (the reference goes on with a NULL accessor), a lookup_key with `${`, a list with a NUL byte at
// the start of a line (the reference reads buf[-1]), more than CL_MAX_RECORDS `record` entries, a table over CL_MAX_TABLE_BYTES,
// and a list whose arena does not fit 32-bit offsets.
#pragma once
#include <cstdint>
#include "dev.hpp"
#include "typeconv.hpp"

namespace flbgpu {

constexpr int CL_MAX_RECORDS = 64;
constexpr uint32_t CL_MAX_TABLE_BYTES = TC_MAX_TABLE_BYTES;      // the LDS budget of typeconv.hpp
constexpr int CL_BLOCK = 256;
constexpr uint32_t CL_LINE = 2048;                 // LINE_SIZE (checklist.h)
constexpr uint32_t CL_BUCKETS = 257;               // partial mode: one per first byte, [256] = `any`
constexpr uint32_t CL_EMPTY = 0xFFFFFFFFu;         // exact mode: the offset word of a free slot

enum { CL_EXACT = 0, CL_PARTIAL = 1 };
enum { CL_VAL_STR = 0, CL_VAL_TRUE = 1, CL_VAL_FALSE = 2, CL_VAL_NIL = 3 };

// per-row flags the size pass keeps (one byte a row)
constexpr uint8_t CLF_DECODED = 1;                 // the decoder hands the row on as a record
constexpr uint8_t CLF_MATCH = 2;                   // its value is on the list
constexpr uint8_t CLF_OK = 4;                      // the encoder takes it (a matched row without this is rolled back)
constexpr uint8_t CLF_SKIP = 8;                    // the decoder steps over it silently (group markers, rows an earlier filter dropped)

// the table in LDS (words):
//   [0] number of `record` pairs    [1] accessor: length of the key name | number of sub-keys << 16 | CL_ACC_INERT
//   [2] byte offset of the key name [3] byte offset of the sub-key list (ra_lds.inc's two words per sub-key)
//   then per `record` pair four words: { key length, byte offset of the key, bytes that go out behind the entries (key STR, value),
//   byte offset of those bytes }, then the sub-key list, then the bytes, each padded to a multiple of 4
constexpr uint32_t CL_HDR_WORDS = 4, CL_REC_WORDS = 4;
constexpr uint32_t CL_ACC_INERT = 1u << 31;

// exact mode, in HBM: slots of four words { hash low, hash high, arena offset | CL_EMPTY, length }, nslots a power of two
// partial mode, in HBM: bucket_off[CL_BUCKETS + 1] into ents[], two words an entry { arena offset, length }
struct ChecklistArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;      // HBM copy of the LDS table
    uint32_t table_bytes;
    int mode, fold;
    const uint8_t *arena;       // the list's bytes
    uint32_t arena_bytes;
    const uint32_t *slots;      // exact
    uint32_t nslots;
    const uint32_t *bucket_off; // partial
    const uint32_t *ents;
    uint32_t nents;
    uint8_t *flags;             // [n]
    uint32_t *enc_len;          // [n] size pass: bytes of the re-encoded record (matched rows the encoder takes)
    uint32_t *len;              // [n] plan: output bytes of the row
    // [0] first row the decoder refuses, [1] first decoded row, [2] first matched row, [3] first matched row the encoder takes,
    // [4] first matched row behind `after` (the rare second look)
    unsigned long long *firsts;
    // [0] decoded, [1] emitted records, [2] matched, [3] rolled back, [4] non-STR values found, [5] rows over 4 GB,
    // [6] rows whose emitted length differs from their sized length
    unsigned long long *counts;
    unsigned long long first_eff;   // plan / emit: the first matched row that leaves something in the output
    unsigned long long after;
    const uint64_t *out_off;
    uint8_t *out;
};

void launch_checklist(const ChecklistArgs &a, bool emit, hipStream_t st);
void launch_checklist_second(const ChecklistArgs &a, hipStream_t st);
void launch_checklist_plan(const ChecklistArgs &a, hipStream_t st);

}  // namespace flbgpu
