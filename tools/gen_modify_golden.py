#!/usr/bin/env python3
"""Records the answers of the real filter_modify for tests/golden/modify_ref_cases.json.

Development machines only: it needs a fluent-bit source tree (--reference, default $REF) and the reference engine of `make -C oracle`
(oracle/_ref/engine).  The plugin's own source is compiled where it lies, as a loadable flb-filter_modify.so in a scratch directory
outside the repository, with the include paths tools/gen_recmod_golden.py uses.  Every case is one chunk through
`engine_host processor -e <.so> <in> <out> --unit modify k=v ...`; the file holds the properties, the input chunk and the output chunk
(base64) and "refused": the filter did not start.  The processor does not hand the callback's answer on, so the file records bytes
only: what the processor hands back is the filter's output -- or, where the filter answered NOTOUCH, the input -- through its group
normalisation (src/flb_processor.c:1811-1852: the records the decoder takes).  A case at which engine_host dies is written as
"crashed": true without bytes; only the cases named in UNDEFINED may end that way, and there is none: every prefix compare of these
cases stays inside its record and inside the re-packed map (what leaves them belongs to the overread counter, not to bytes).

Not recorded, because the reference misbehaves there: a Condition of one token (it reads past its split list),
`Hard_copy k k` (a map header one larger than its entries), a condition pattern Onigmo refuses (the first record dereferences the
NULL regex); and an empty fixstr key under a prefix rule (Remove_wildcard, Move_to_*): msgpack-c's
unpacker gives a zero-length fixstr the pointer of the item it read last (unpack_template.h, _str_zero pushes the stale `n`), so the
compare runs over unrelated bytes, or over NULL.  The cases are hand-written and named; tests/test_modify_ref.py lists the names it requires."""
import argparse
import base64
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402
from gen_recmod_golden import includes  # noqa: E402

R = synth.Raw
UNDEFINED = ()
TAIL = ("tail", "t" * 48)                      # closes a record in which a key shorter than a prefix rule occurs


def rec(body, sec=0, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def kv(*items):
    return synth.KV(list(items))


def binkey(b):
    return R(b"\xc4" + bytes([len(b)]) + b)


def str8(b):
    return R(b"\xd9" + bytes([len(b)]) + b)


def str16(b):
    return R(b"\xda" + struct.pack(">H", len(b)) + b)


def str32(b):
    return R(b"\xdb" + struct.pack(">I", len(b)) + b)


def grid(nks, nts):
    """records with nk entries under "k" and nt entries under "t", other entries between them"""
    out, i = b"", 0
    for nk in nks:
        for nt in nts:
            i += 1
            items = [("a", 1)] + [("k", "kv%d" % j) for j in range(nk)] + [("m", 2)] + [("t", "tv%d" % j) for j in range(nt)] + [("z", 3)]
            out += rec(kv(*items), i, nk * 10 + nt)
    return out


KEYS = kv(("k", 1), (str8(b"k"), 2), (str16(b"k"), 3), (str32(b"k"), 4), (binkey(b"k"), 5), (7, 6), (None, 7), (True, 8), (False, 9),
          ("z", 10))
NONCANON = R(b"\xde\x00\x04" + b"\xda\x00\x03abc" + b"\xd1\x00\x07" + b"\xd9\x01x" + b"\xde\x00\x01\xd9\x01q\xd0\x05" +
             b"\xa1y\xd2\x00\x00\x00\x01" + b"\xc5\x00\x02kb" + b"\xdb\x00\x00\x00\x02hi")
NONCANON2 = R(b"\xde\x00\x03" + b"\xda\x00\x03abc" + b"\xd1\x00\x07" + b"\xa1y\xde\x00\x01\xd9\x01q\xd0\x05" + b"\xc5\x00\x02kb\xcd\x00\x01")
VALUE_TYPES = [("s", "true"), ("b", R(b"\xc4\x04true")), ("o", True), ("i", 1), ("m", kv(("true", 1))), ("f", False), ("n", None)]


def cases():
    c = []

    def add(name, props, data):
        c.append(dict(name=name, props=[list(p) for p in props], data=data))
    # ---- the eleven rules with 0, 1 and 2 entries under the key (and, for the two-token rules, under the target)
    for name in ("Remove", "Remove_wildcard", "Remove_regex", "Move_to_start", "Move_to_end"):
        add("rule_%s_012" % name.lower(), [(name, "^k$" if name == "Remove_regex" else "k")], grid((0, 1, 2), (1,)))
    for name in ("Rename", "Hard_rename", "Copy", "Hard_copy"):
        add("rule_%s_grid" % name.lower(), [(name, "k t")], grid((0, 1, 2), (0, 1, 2)))
    add("rule_add_012", [("Add", "k new")], grid((0, 1, 2), (1,)))
    add("rule_add_if_not_present_012", [("Add_if_not_present", "k new")], grid((0, 1, 2), (1,)))
    add("rule_set_012", [("Set", "k new")], grid((0, 1, 2), (1,)))
    add("rename_onto_existing_key", [("Rename", "a b")], rec(kv(("a", 1), ("b", 2)), 1) + rec(kv(("a", 1), ("c", 2)), 2))
    add("copy_two_sources", [("Copy", "a b")], rec(kv(("a", 1), ("x", 0), ("a", 2)), 1) + rec(kv(("x", 0), ("a", 2), ("y", 3)), 2))
    add("hard_copy_target_before_and_behind", [("Hard_copy", "k t")],
        rec(kv(("t", "old"), ("a", 1), ("k", "src"), ("z", 2)), 1) + rec(kv(("a", 1), ("k", "src"), ("z", 2), ("t", "old"), ("y", 3)), 2) +
        rec(kv(("t", "old"), ("k", "src"), ("t", "old2")), 3) + rec(kv(("k", "src")), 4))
    add("hard_rename_two_targets", [("Hard_rename", "k t")],
        rec(kv(("t", 1), ("k", 2), ("a", 0), ("t", 3)), 1) + rec(kv(("k", 1), ("t", 2), ("k", 3), ("t", 4), (binkey(b"t"), 5)), 2))
    add("set_over_duplicates", [("Set", "k v")],
        rec(kv(("k", 1), ("a", 2), (binkey(b"k"), 3), ("k", 4), ("z", 5)), 1) + rec(kv(("a", 2)), 2))
    inter = kv(("x1", 1), ("a", 2), ("x2", 3), ("b", 4), (binkey(b"x3"), 5), ("c", 6))
    add("move_to_start_stable", [("Move_to_start", "x")], rec(inter, 1))
    add("move_to_end_stable", [("Move_to_end", "x")], rec(inter, 1))
    pref = kv(("ab", 1), ("xab", 2), ("abc", 3), ("a", 4), ("b", 5), (binkey(b"abd"), 6), TAIL)
    for name in ("Remove_wildcard", "Move_to_start", "Move_to_end"):
        add("prefix_%s" % name.lower(), [(name, "ab")], rec(pref, 1))
    add("three_tokens_set_is_rename", [("Set", "a b c")], rec(kv(("a", 1), ("b", 2)), 1) + rec(kv(("a", 1), ("c", 2)), 2) + rec(kv(("b", 1)), 3))
    add("three_tokens_remove_is_rename", [("Remove", "a b c")], rec(kv(("a", 1), ("b", 2)), 1))
    add("rules_in_sequence", [("Rename", "a b"), ("Copy", "b c"), ("Remove", "z"), ("Add", "b 1"), ("Hard_rename", "c a"), ("Move_to_start", "a")],
        rec(kv(("a", 1), ("z", 2), ("y", 3)), 1) + rec(kv(("b", 1), ("a", 2)), 2))
    # ---- the ten conditions, true and false in one chunk
    hit = [("Add", "hit 1")]
    k_v, k_w, no_k = rec(kv(("k", "v"), ("o", 1)), 1), rec(kv(("k", "w"), ("o", 1)), 2), rec(kv(("o", 1)), 3)
    add("cond_key_exists", [("Condition", "Key_exists k")] + hit, k_v + no_k)
    add("cond_key_does_not_exist", [("Condition", "Key_does_not_exist k")] + hit, k_v + no_k)
    add("cond_a_key_matches", [("Condition", "A_key_matches ^k[0-9]$")] + hit, rec(kv(("k", 1), ("k1", 2)), 1) + rec(kv(("k", 1), ("k12", 2)), 2))
    add("cond_no_key_matches", [("Condition", "No_key_matches ^k[0-9]$")] + hit, rec(kv(("k", 1), ("k1", 2)), 1) + rec(kv(("k", 1), ("k12", 2)), 2))
    add("cond_key_value_equals", [("Condition", "Key_value_equals k v")] + hit, k_v + k_w + no_k)
    add("cond_key_value_does_not_equal", [("Condition", "Key_value_does_not_equal k v")] + hit, k_v + k_w + no_k)
    add("cond_key_value_matches", [("Condition", "Key_value_matches k ^v")] + hit, k_v + k_w + no_k)
    add("cond_key_value_does_not_match", [("Condition", "Key_value_does_not_match k ^v")] + hit, k_v + k_w + no_k)
    mk = rec(kv(("k1", "v1"), ("o", "x"), ("k2", "v2")), 1) + rec(kv(("k1", "v1"), ("k2", "x")), 2) + rec(kv(("o", 1)), 3) + \
        rec(kv(("k1", 5)), 4)
    add("cond_matching_keys_have_matching_values", [("Condition", "Matching_keys_have_matching_values ^k ^v")] + hit, mk)
    add("cond_matching_keys_do_not_have_matching_values", [("Condition", "Matching_keys_do_not_have_matching_values ^k ^v")] + hit, mk)
    add("cond_key_twice_last_wins", [("Condition", "Key_value_equals k v")] + hit,
        rec(kv(("k", "v"), ("k", "w")), 1) + rec(kv(("k", "w"), ("k", "v")), 2) + rec(kv(("k", "w"), ("k", "v"), (binkey(b"k"), "w")), 3))
    add("cond_key_bin_only", [("Condition", "Key_exists k")] + hit,
        rec(kv((binkey(b"k"), 1)), 1) + rec(kv((str8(b"k"), 1)), 2) + rec(kv((binkey(b"k"), 1), (str16(b"k"), 2)), 3))
    types = b"".join(rec(kv(("k", v), ("o", 1)), i) for i, (_, v) in enumerate(VALUE_TYPES))
    add("cond_equals_value_types", [("Condition", "Key_value_equals k true")] + hit, types)
    add("cond_does_not_equal_value_types", [("Condition", "Key_value_does_not_equal k true")] + hit, types)
    add("cond_matches_value_types", [("Condition", "Key_value_matches k ^true$")] + hit, types)
    add("cond_does_not_match_value_types", [("Condition", "Key_value_does_not_match k ^true$")] + hit, types)
    add("cond_matches_false", [("Condition", "Key_value_matches k ^false$")] + hit, types)
    key_types = b"".join(rec(kv((k, 1), ("o", 1)), i) for i, k in enumerate(["true", binkey(b"true"), True, False, 1, None, str8(b"true")]))
    add("cond_a_key_matches_key_types", [("Condition", "A_key_matches ^true$")] + hit, key_types)
    add("cond_matching_keys_value_types", [("Condition", "Matching_keys_have_matching_values ^. ^true$")] + hit,
        b"".join(rec(kv((n, v)), i) for i, (n, v) in enumerate(VALUE_TYPES)) + rec(kv((True, True)), 9) + rec(kv((True, 1)), 10))
    acc = rec(kv(("a", kv(("b", [1, 2])))), 1) + rec(kv(("a", kv(("b", 1)))), 2) + rec(kv(("a", kv(("c", 1)))), 3) + rec(kv(("a", 1)), 4) + \
        rec(kv(("a", kv(("b", [kv(("c", 1))])))), 5)
    add("cond_accessor_ends_on_index", [("Condition", "Key_exists $a['b'][0]")] + hit, acc)
    add("cond_accessor_ends_on_index_negated", [("Condition", "Key_does_not_exist $a['b'][0]")] + hit, acc)
    add("cond_accessor_ends_on_key", [("Condition", "Key_exists $a['b']")] + hit, acc)
    add("cond_accessor_index_then_key", [("Condition", "Key_exists $a['b'][0]['c']")] + hit, acc)
    add("cond_accessor_value_equals", [("Condition", "Key_value_equals $a['b'] x")] + hit,
        rec(kv(("a", kv(("b", "x")))), 1) + rec(kv(("a", kv(("b", "y")))), 2) + rec(kv(("a", kv(("b", "y"), ("b", "x")))), 3))
    add("cond_two_one_false", [("Condition", "Key_exists k"), ("Condition", "Key_value_equals o x")] + hit,
        rec(kv(("k", 1), ("o", "x")), 1) + rec(kv(("k", 1), ("o", "y")), 2) + rec(kv(("o", "x")), 3))
    add("cond_on_original_record", [("Condition", "Key_exists k"), ("Remove", "k"), ("Add", "k again")], k_v + no_k)
    # ---- key and value encodings
    add("keys_remove", [("Remove", "k")], rec(KEYS, 1))
    add("keys_rename_other", [("Rename", "z y")], rec(KEYS, 1))
    add("keys_rename", [("Rename", "k y")], rec(KEYS, 1))
    add("keys_remove_regex_true", [("Remove_regex", "^true$")], rec(KEYS, 1))
    add("keys_remove_regex_k", [("Remove_regex", "^k$")], rec(KEYS, 1))
    add("keys_move_to_end", [("Move_to_end", "k")], rec(KEYS, 1))
    add("keys_set", [("Set", "k v")], rec(KEYS, 1))
    nul = kv((b"a\0b", 1), ("a", 2), (b"a\0", 3), (binkey(b"a\0b"), 4), ("z", 5), TAIL)
    add("key_nul_remove", [("Remove", "a")], rec(nul, 1))
    add("key_nul_wildcard", [("Remove_wildcard", "a")], rec(nul, 1))
    add("key_nul_regex", [("Remove_regex", "^a.b$")], rec(nul, 1))
    m16 = R(b"\xde\x00\x02\xa1x\x01\xa1y\x02")
    m32 = R(b"\xdf\x00\x00\x00\x02\xa1x\x01\xa1y\x02")
    add("body_map16", [("Remove", "x")], rec(m16, 1) + rec(R(b"\xde\x00\x01\xa1y\x02"), 2))
    add("body_map32", [("Remove", "x")], rec(m32, 1) + rec(R(b"\xdf\x00\x00\x00\x01\xa1y\x02"), 2))
    add("non_canonical_entries", [("Remove", "x")], rec(NONCANON, 1) + rec(NONCANON2, 2))
    add("non_canonical_none_applied", [("Remove", "absent")], rec(NONCANON, 1) + rec(NONCANON2, 2))
    add("non_canonical_metadata", [("Remove", "x")],
        rec(kv(("x", 1), ("y", 2)), 5, 6, kv(("m", 1), ("z", [1, 2]))) +
        synth.mp([[synth.ext_ts(7, 8), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("x", 1), ("y", 2))]) +
        synth.mp([[synth.ext_ts(9, 1), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("y", 2))]))
    # ---- the prefix test on a key shorter than the rule: the bytes behind the key take part (all inside the record / the re-pack)
    short = rec(kv(("a", 98), ("z", 1), TAIL), 1) + rec(kv(("a", 99), ("z", 1), TAIL), 2) + rec(kv(("a", "b"), TAIL), 3)
    add("prefix_short_key_before_rule", [("Remove_wildcard", "ab")], short)
    add("prefix_short_key_after_set", [("Set", "q w"), ("Remove_wildcard", "ab")], short)
    ints = rec(kv(("a", 98), (99, 100), ("z", 1), TAIL), 1) + rec(kv(("a", 98), (99, 101), ("z", 1), TAIL), 2)
    add("prefix_short_key_through_entries", [("Move_to_end", "abcd")], ints)
    add("prefix_short_key_through_entries_after_set", [("Set", "q w"), ("Move_to_end", "abcd")], ints)
    # the value d0 62 is 62 in the re-pack: a miss on the record's bytes, a hit once a rule has applied
    wide = rec(kv(("a", R(b"\xd0\x62")), ("z", 1), TAIL), 1)
    add("prefix_short_key_repack_changes_bytes", [("Remove_wildcard", "ab")], wide)
    add("prefix_short_key_repack_changes_bytes_after_set", [("Set", "q w"), ("Remove_wildcard", "ab")], wide)
    # the entry behind the key goes: the compare runs into the entry that follows it in the re-pack
    add("prefix_short_key_behind_removed_entry", [("Remove", "gone"), ("Move_to_start", "abc")],
        rec(kv(("z", 1), ("a", 98), ("gone", 1), (99, 2), TAIL), 1) + rec(kv(("z", 1), ("a", 98), (99, 2), TAIL), 2) +
        rec(kv(("z", 1), ("a", 98), ("gone", 1), (100, 2), TAIL), 3))
    # ---- call level
    one = [("Set", "k x")]
    add("legacy_rows", one,
        synth.mp([1700000000, kv(("k", 1))]) + synth.mp([1700000000.25, kv(("k", 2))]) +
        synth.mp([R(b"\xd7\x00" + struct.pack(">II", 5, 6)), kv(("k", 4))]) + synth.mp([0, kv(("k", 5))]))
    add("group_markers", one,
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), kv(("g", 1))], kv(("r", 1))]) + rec(kv(("k", 1)), 4) +
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xfe\x00\x00\x00\x00"), {}], {}]) + rec(kv(("k", 2)), 5))
    add("group_markers_nothing_applies", [("Remove", "absent")],
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), kv(("g", 1))], kv(("r", 1))]) + rec(kv(("k", 1)), 4) +
        synth.mp([[R(b"\xd7\x00\xff\xff\xff\xfe\x00\x00\x00\x00"), {}], {}]) + rec(kv(("k", 2)), 5))
    add("bad_time", one,
        synth.mp([2 ** 32 - 1, kv(("k", 1))]) + synth.mp([2 ** 32, kv(("k", 2), ("y", R(b"\xd0\x05")))]) +
        synth.mp([2 ** 40, kv(("k", 3))]) + rec(kv(("k", 4)), 3))
    add("bad_time_only", one, synth.mp([2 ** 32, kv(("k", 2))]) + synth.mp([2 ** 40, kv(("k", 3))]))
    bad = synth.mp([[synth.ext_ts(3), {}], "text"])
    add("non_map_body_first", one, bad + rec(kv(("k", 1)), 4))
    add("non_map_body_middle", one, rec(kv(("k", 1)), 1) + rec(kv(("y", 2)), 2) + bad + rec(kv(("k", 1)), 4))
    add("garbage_reserved_byte", one, rec(kv(("k", 1), ("y", 2)), 1) + b"\xc1" + rec(kv(("k", 1)), 2))
    add("garbage_reserved_byte_last", one, rec(kv(("k", 1), ("y", 2)), 1) + b"\xc1")
    add("garbage_cut_record", one, rec(kv(("k", 2)), 1) + rec(kv(("k", "long value")), 2)[:-4])
    # cut on a field boundary, and behind a header whose payload is missing altogether: msgpack-c has consumed all it was given
    add("garbage_cut_on_field_boundary", one, rec(kv(("k", 2)), 1) + rec(kv(("k", "long value"), ("y", 1)), 2)[:-3])
    add("garbage_cut_behind_header", one, rec(kv(("k", 2)), 1) + rec(kv(("k", "long value"), ("y", 1)), 2)[:-2])
    add("garbage_cut_behind_length_field", one, rec(kv(("k", 2)), 1) + rec(kv(("k", R(b"\xd9\x0along value"))), 2)[:-10])
    add("garbage_cut_in_length_field", one, rec(kv(("k", 2)), 1) + rec(kv(("k", R(b"\xda\x00\x0along value"))), 2)[:-11])
    add("garbage_cut_record_nothing_applies", [("Remove", "absent")], rec(kv(("k", 2)), 1) + rec(kv(("k", "long value")), 2)[:-4])
    add("nothing_applies", [("Remove", "absent"), ("Rename", "absent other"), ("Condition", "Key_exists k")],
        rec(kv(("k", 1)), 1) + rec(kv(("y", R(b"\xd0\x05"))), 2) + rec({}, 3))
    add("empty_map_add", [("Add", "k v")], rec({}, 1) + rec(R(b"\xde\x00\x00"), 2) + rec(kv(("k", 1)), 3))
    add("empty_map_remove", [("Remove", "k")], rec({}, 1) + rec(kv(("k", 1)), 3))
    # ---- front end
    ab = rec(kv(("a", 1), ("b", 2)), 5, 6)
    add("property_names_other_case", [("SET", "a x"), ("condition", "KEY_EXISTS a"), ("remove_WILDCARD", "b")], ab)
    add("unknown_property", [("Set", "a x"), ("Frobnicate", "a")], ab)
    add("four_tokens", [("Set", "a b c d")], ab)
    add("repeated_rule_name", [("Add", "c 1"), ("Add", "d 2"), ("Remove", "a"), ("Remove", "b")], ab)
    add("repeated_condition", [("Condition", "Key_exists a"), ("Condition", "Key_exists c"), ("Add", "d 2")], ab + rec(kv(("a", 1), ("c", 2))))
    add("quoted_tokens", [("Set", '"a key" "a value"'), ("Rename", "a 'b c'")], ab)
    add("one_token_two_token_rule", [("Set", "a")], ab)
    add("two_tokens_one_token_rule", [("Remove", "a b")], ab)
    add("unknown_condition", [("Condition", "Key_is_nice a"), ("Set", "a x")], ab)
    add("no_rules", [], ab)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REF"), help="fluent-bit source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "modify_ref_cases.json"))
    a = ap.parse_args()
    engine = os.path.join(ROOT, "oracle", "_ref", "engine")
    host = os.path.join(engine, "engine_host")
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "plugins", "filter_modify")):
        sys.exit("need --reference <fluent-bit source tree>")
    if not os.path.exists(host):
        sys.exit("build the reference engine first: make -C oracle")
    out = []
    with tempfile.TemporaryDirectory(prefix="modify_golden_") as tmp:
        so = os.path.join(tmp, "flb-filter_modify.so")
        src = os.path.join(a.reference, "plugins", "filter_modify")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-D__FLB_FILENAME__=__FILE__"] + includes(a.reference, engine) +
                       ["-I" + os.path.join(a.reference, "lib"), "-I" + src, "-o", so, os.path.join(src, "modify.c")], check=True)
        for c in cases():
            e = dict(name=c["name"], props=c["props"], **{"in": base64.b64encode(c["data"]).decode()})
            fin, fout = os.path.join(tmp, "in.mp"), os.path.join(tmp, "out.mp")
            with open(fin, "wb") as f:
                f.write(c["data"])
            if os.path.exists(fout):
                os.unlink(fout)
            cmd = [host, "processor", "-e", so, fin, fout, "--unit", "modify"] + ["%s=%s" % (k, v) for k, v in c["props"]]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
            if r.returncode < 0 or r.returncode >= 128:
                if c["name"] not in UNDEFINED:
                    sys.exit("%s: engine_host died (%d): %s" % (c["name"], r.returncode, r.stderr.decode()[-400:]))
                e["crashed"] = True
            elif not lines:
                # a property the config map refuses is reported before the processor starts
                if r.returncode == 3 or b"refused" in r.stderr:
                    e["refused"] = True
                else:
                    sys.exit("%s: engine_host said nothing (exit %d): %s" % (c["name"], r.returncode, r.stderr.decode()[-400:]))
            elif not json.loads(lines[-1]).get("init", True):
                e["refused"] = True
            else:
                e["out"] = base64.b64encode(open(fout, "rb").read()).decode()
            if c["name"] in UNDEFINED:
                e["undefined"] = True
            out.append(e)
    with open(a.out, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]}\n")
    print("%d cases, %d bytes -> %s" % (len(out), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()
