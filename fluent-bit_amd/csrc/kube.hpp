// kube.hpp -- filter_kubernetes' per-record half as the device sees it (kube.cpp builds it, kube_kernels.inc runs it)
// plugins/filter_kubernetes/kubernetes.c:112-137 (get_stream), 139-161 (value_trim_size), 163-247 (merge_log_handler), 318-644
// (pack_map_content), 646-872 (one call).  The metadata half (kube_meta.c) stays with the caller: the filter takes the cache entries
// flb_kube_meta_get would answer a hit with (flbgpu_kubernetes_set_meta) or builds the pod entry from the tag (set_tag).
//
// Limits and refusals at create time (DESIGN 8 lists them): an unknown property, a bool that is none, use_journal on, dummy_meta on,
// merge_parser, regex_parser, a merge_log_key of KB_MAX_MERGE_KEY bytes or more, `${` in a value.
#pragma once
#include <cstdint>
#include "dev.hpp"

namespace flbgpu {

constexpr int KB_BLOCK = 256;
constexpr uint32_t KB_MAX_MERGE_KEY = 32768;
constexpr uint32_t KB_MAX_ENTRY = 1u << 20;
// The packed JSON map is unpacked again with results unchecked (:405-412, :493-496).  The stock build compiles msgpack-c with
// MSGPACK_EMBED_STACK_SIZE=64 (cmake/msgpack.cmake:11; the header's own default is 32), and the recording of the real plugin pins it:
// the map with 63 more containers open inside a value merges, with 64 it has no entries.
constexpr uint32_t KB_UNPACK_OPEN = 64;
// LDS: the table (KB_HDR_WORDS words and the packed merge_log_key, under 33 KB) and -- when it fits the budget -- the tail every record
// gets appended.  The default budget keeps table + tail under 48 KB, three workgroups a CU at the worst.
constexpr uint32_t KB_LDS_BLOB_DEFAULT = 15360;

// the passes of k_kube
enum { KB_SIZE = 0, KB_EMIT = 1 };
// configuration flags (table word 0)
constexpr uint32_t KBF_MERGE_LOG = 1u, KBF_KEEP_LOG = 2u, KBF_TRIM = 4u, KBF_MERGE_KEY = 8u, KBF_EXCL_STDOUT = 16u, KBF_EXCL_STDERR = 32u;
constexpr uint32_t KBF_TAIL_PAIRS_SHIFT = 8;      // bits 8-9: the pairs of the tail (kubernetes, kubernetes_namespace): 0, 1 or 2
// the table in LDS (words): [0] flags  [1] bytes of the packed merge_log_key (STR header and name)  [2] bytes of the tail
// [3] 1: the tail stands in LDS behind the table; then the packed merge_log_key, padded to a multiple of 4
constexpr uint32_t KB_HDR_WORDS = 4;
// a row's state byte, kept from the size pass for the emit pass
constexpr uint8_t KBS_OUT = 1;            // the record goes out
constexpr uint8_t KBS_DEFER = 2;          // its JSON needs the exact instantiation (nesting past the register walker, a hard decimal)
constexpr uint8_t KBS_PARSED = 4;         // its `log` is a STR that flb_pack_json_recs took: MERGE_PARSED
constexpr uint8_t KBS_EMPTY = 8;          // ... whose packed map has no entries to merge

struct KubeArgs {
    const uint8_t *data;
    const uint64_t *row_off;
    uint64_t n;
    const uint32_t *table;      // HBM copy of the LDS table
    uint32_t table_bytes;
    const uint8_t *tail;        // "kubernetes" + pod map + "kubernetes_namespace" + namespace map, as every record ends
    uint32_t tail_bytes;
    uint32_t tail_in_lds;
    uint8_t *state;             // [n]
    uint32_t *len;              // [n] size pass: output bytes of the row, the tail included
    // [0] first row the decoder refuses, [1] first row whose time the encoder refuses
    unsigned long long *firsts;
    // [0] records decoded, [1] records merged, [2] records excluded, [3] records under a counted deviation, [4] records emitted,
    // [5] rows over 4 GB, [6] rows whose emitted length differs from their sized length, [7] rows left to the exact instantiation
    unsigned long long *counts;
    const uint64_t *out_off;
    uint8_t *out;
};

// exact: the instantiation with the wide bit stack and the big-integer decimals, over the rows the first one deferred
void launch_kube(const KubeArgs &a, int pass, bool exact, hipStream_t st);

}  // namespace flbgpu
