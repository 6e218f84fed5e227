// throttle.hpp -- filter_throttle_size's program and window state as the device sees them (throttle.cpp builds them,
// throttle_kernels.inc runs them).  plugins/filter_throttle_size/throttle_size.c:308-433 (throttle_data_by_size), 169-192 (the ticker),
// size_window.h:59-91 (add_new_pane, add_load).  filter_throttle (plugins/filter_throttle/throttle.c, window.c) has no device state:
// its window lives on the host and the device only copies the first K records (throttle.cpp).
//
// Refusals at create time (DESIGN 8 lists them): a path table over TC_MAX_TABLE_BYTES.
#pragma once
#include <cstdint>
#include "dev.hpp"
#include "typeconv.hpp"

namespace flbgpu {

constexpr int TSZ_BLOCK = 256;
constexpr int TSZ_MAX_PARTS = 21;                   // flb_utils_split(str, '|', 20): twenty parts and the rest of the line
constexpr uint32_t TSZ_EXEMPT = 0xFFFFFFFFu;        // the record is kept and no window is touched (name or log field missing)
constexpr uint32_t TSZ_UNSEEN = 0xFFFFFFFEu;        // a row the decoder's loop never hands on (group marker, dropped row): not kept
constexpr uint32_t TSZ_NONE = 0xFFFFFFFDu;          // the dictionary was full: the host grows it and the pass runs again
constexpr uint32_t TSZ_WAVE_MIN = 64;               // segments of this many rows take a wave (test switch FLBGPU_TSZ_WAVE_MIN)

// the table in LDS (words): [0] parts of name_field, [1] parts of log_field, then per part -- the name's first -- { length, byte
// offset }, then the parts' bytes, each padded to a multiple of 4
constexpr uint32_t TSZ_HDR_WORDS = 2;

// the windows, columns by window id (= the name's number in the dictionary)
struct TszWindows {
    uint32_t *exists;               // [cap]
    unsigned long long *total;      // [cap]
    long long *timestamp;           // [cap]
    int32_t *head, *tail;           // [cap]
    long long *pane_ts;             // [cap][window]
    unsigned long long *pane_size;  // [cap][window]
    uint32_t window;                // panes per window
};

struct TszArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;          // HBM copy of the LDS table
    uint32_t table_bytes;
    L2mTable t;                     // the names
    uint64_t hash_mask;             // FLBGPU_TSZ_HASH_BITS: the bits of a name's hash that are kept
    uint32_t *wid;                  // [n] window id, TSZ_EXEMPT, TSZ_UNSEEN or TSZ_NONE
    unsigned long long *load;       // [n]; nullptr (filter_throttle): no name, no load, wid[r] = 1 for a record and 0 for any other row
    uint32_t *len;                  // [n] the record's bytes (0 for a row that is never handed on)
    // [0] first row the decoder refuses
    unsigned long long *firsts;
    double rate;                    // for a record with an empty name: it is judged alone, in the extraction
    uint32_t window;
    // [0] records, [1] exempt records, [2] rows over 4 GB, [3] throttled records, [4] records with an empty name that were dropped
    unsigned long long *counts;
};

struct TszAdmitArgs {
    TszWindows w;
    const uint32_t *keys;           // [m] window ids, sorted (stable)
    const uint32_t *rows;           // [m] the row of each
    uint64_t m;
    const unsigned long long *load; // [n] by row
    uint32_t *len;                  // [n] by row: set to 0 where the record is dropped
    double rate;
    long long now;                  // the timestamp of a window created in this call
    uint32_t wave_min;
    // [0] records dropped, [1] windows created
    unsigned long long *counts;
    // work: the list of long segments (each by the index of its first sorted row)
    unsigned int *nheavy;
    uint32_t *heavy;                // [m]
};

struct TszTickArgs {
    TszWindows w;
    uint32_t nids;
    long long ts, threshold;        // the pane's timestamp; (long) (ts - window_time_duration)
    // [0] windows live after the tick, [1] windows deleted by it
    unsigned long long *counts;
};

void launch_tsz_extract(const TszArgs &a, hipStream_t st);
size_t tsz_order_bytes(uint64_t n);
// the throttled rows in (window id, row) order and the empty list of long segments (false: the sort failed); then the admission:
// wave false -- a lane per short segment, the long ones listed --, wave true -- a wave per listed segment
bool launch_tsz_order(TszAdmitArgs &a, const uint32_t *wid, uint64_t n, uint32_t nids, void *work, size_t work_bytes, hipStream_t st);
void launch_tsz_admit(const TszAdmitArgs &a, bool wave, hipStream_t st);
void launch_tsz_tick(const TszTickArgs &a, hipStream_t st);
void launch_thr_first(uint32_t *len, const uint64_t *idx, uint64_t K, uint64_t n, hipStream_t st);

}  // namespace flbgpu
