// parser_words.hpp -- the slots of the counter block that filter_parser and filter_grep keep on the device and mirror in page-locked
// host memory (flbgpu.cpp MiscWords::counts; the kernels reach it through their arguments' `counts`, `len_stat`, `err` ... pointers).
// Grouped by who gives a slot its meaning.  Where one index has two names, the two never live in the same call: a call zeroes the
// block, and the passes that share an index never both run in it (or the later one zeroes the slot first: the decoders).
#pragma once

namespace flbgpu {

enum {
    // ---- every pass
    MW_DECODED = 0,         // records the decoder took: the filter's records in
    // ---- filter_parser's size pass (k_parser_reg / k_parser_tile / the phase kernels, k_scan)
    MW_EMITTED = 1,         // records with an output, counted by the scan: what flb_mp_count_log_records would report
    MW_GENERIC = 2,         // rows outside the fast shape, flagged RF_GENERIC for k_parser_generic
    MW_EXACT = 3,           // rows flagged RF_EXACT for k_parser_emit_exact
    MW_FINISH = 8,          // rows left to k_parser_finish: a time text for the strptime interpreter, sizes that depend on the record's bytes
    MW_SLOW = 9,            // values the forward walk from boundary 0 did not settle (the reverse pass took them)
    MW_NEEDLOC = 10,        // rows the call-free kernel only flagged (RF_NEEDLOC): left to the fix-up launch
    MW_FIX_SPAN = 11,       // n - (the first such row that no wave listed): where the fix-up launch starts
    MW_FIX_COUNT = 12,      // ParserMatchArgs::fix_count
    MW_TIME_MARKER = 14,    // parsed times the next filter's decoder reads as a group marker: written, not counted as records out
    MW_LEN_STEPS = 16,      // ParserMatchArgs::len_stat[0]: what the register kernel's walk steps through in chunk order
    MW_LEN_BYTES = 17,      // ParserMatchArgs::len_stat[1]: what the rows hold
    // ---- the decoders (k_parser_dec; they zero their two slots themselves, after the size pass has read MW_NEEDLOC and MW_FIX_SPAN)
    MW_DEC_OVER = 10,       // DecArgs::err: rows that outgrew the decoders' scratch
    MW_DEC_ROWS = MW_DEC_OVER + 1,      // DecArgs::ndec: rows the size pass handled
    // ---- filter_grep's pass (k_grep_match, k_grep_lane)
    MW_KEPT = 1,            // records the rules keep
    MW_LANE_BYTES = 10,     // GrepLaneArgs::words[0]: bytes the one-pass kernel wrote (two instances: what the second keeps)
    MW_LANE_FAIL = MW_LANE_BYTES + 1,   // GrepLaneArgs::words[1]: workgroups without room for their output / that gave up waiting (<< 32)
    MW_LANE_TICKET = 12,    // GrepLaneArgs::ticket
    MW_TILE_MAX = 13,       // lane_geometry: the longest run of 64 rows
    // ---- two filter_grep instances as one pass (k_grep_lane with GrepLaneArgs::two)
    MW_KEPT2 = 2,           // records the second instance keeps
    MW_BYTES1 = 3,          // bytes the first instance keeps
    // ---- the fused parser + grep pair (the size pass in pair mode, k_pg_decide, k_pg_emit)
    MW_PG_BYTES = 4,        // bytes filter_parser would have written
    MW_PG_KEEP = 5,         // records filter_grep keeps
    MW_PG_OUT = 6,          // records filter_parser emits
    MW_PG_PENDING = 7,      // rows the inline evaluation left open for k_pg_decide
    MW_PG_TIME_FAIL = 13,   // kept records whose time k_pg_emit could not settle (a text its plan refuses, a time the encoder refuses)
    MW_PG_LEFT = 15,        // kept records the plain build of k_pg_emit left to the general build
    MW_N = 18
};

}  // namespace flbgpu
