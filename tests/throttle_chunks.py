"""The cases of tools/gen_throttle_golden.py and the record builders of the throttle tests, kept apart so that the chunks can be
built and looked at without a device.  A case is (name, props, steps); a step is ("now", T), ("tick", T) or ("chunk", bytes)."""
import random
import struct

import synth
from checklist_chunks import GROUP_END, GROUP_START, R, f32, kv, rec, sv  # noqa: F401

T0 = 1000                   # the scripts' clock starts here
DEVIATES = ("nul_in_name_alone", "nul_in_name_beside_its_prefix")


def bv(b):
    """a BIN of any bytes"""
    b = bytes(b)
    n = len(b)
    h = b"\xc4" + bytes([n]) if n < 256 else b"\xc5" + struct.pack(">H", n) if n < 65536 else b"\xc6" + struct.pack(">I", n)
    return R(h + b)


def str16(b):
    return R(b"\xda" + struct.pack(">H", len(b)) + bytes(b))


def str32(b):
    return R(b"\xdb" + struct.pack(">I", len(b)) + bytes(b))


def simple(log, stream, i, key="log", skey="stream"):
    """the flat record of tests/runtime/filter_throttle_size.c"""
    return synth.mp([1700000060.0, kv((key, log), (skey, stream), ("time", "2024-05-06T07:08:09.000000001Z"), ("value", str(i)))])


def nested(log, pod, i, wrapper="logwrapper", lkey="log", kube="kubernetes", pkey="pod_name", pad=None):
    """the nested record of tests/runtime/filter_throttle_size.c"""
    return synth.mp([1700000413.25, kv((wrapper, kv((lkey, log), ("extra", "field"))), ("stream", "stdout"),
                                           ("time", "2024-05-06T07:08:09.000000001Z"),
                                           (kube, kv((pkey, pod), ("namespace_name", "ns"), ("pod_id", "00000000-1111-2222-3333-444444444444"),
                                                     ("labels", kv(("run", "web"))), ("host", "node-1"), ("container_name", "web"),
                                                     ("docker_id", "0123456789abcdef" * 4))),
                                           ("va", str(i)), *([("pad", "p" * pad)] if pad is not None else []))])


def named(name, load, sec=1, extra=()):
    """{n: name, log: <load bytes>}: the record of most cases (name_field n, log_field log)"""
    return rec(kv(("n", name), ("log", "x" * load), *extra), sec)


NL = [("name_field", "n"), ("log_field", "log")]


def size_cases():
    c = []

    def add(name, props, steps):
        c.append((name, [tuple(p) for p in props], list(steps)))

    def chunks(recs, per):
        return [("chunk", b"".join(recs[i:i + per])) for i in range(0, len(recs), per)]
    start = [("now", T0), ("tick", T0)]
    # ---- tests/runtime/filter_throttle_size.c: the four tests' records in their order, a call per record and then per pair
    base = [("rate", "10"), ("window", "30"), ("interval", "3s"), ("window_time_duration", "10s")]
    m32, m11, m6, m180 = "a" * 32, "b" * 11, "c" * 6, "d" * 180
    r = []
    for i in range(9):
        r += [simple(m32, "stdout", i), simple(m32, "stderr", i)]
    r += [simple(m32, "stdout", 9), simple(m32, "stderr", 9), simple(m11, "stdout", 10), simple(m11, "stderr", 10)]
    for i in range(2):
        r += [simple(m180, "stdout", i + 11, key="msg"), simple(m180, "stderr", i + 11, key="msg")]
    for i in range(2):
        r += [simple(m180, "stdout", i + 13, skey="source"), simple(m180, "stderr", i + 13, skey="source")]
    p = base + [("print_status", "true"), ("log_field", "log"), ("name_field", "stream")]
    add("rt_simple_log", p, start + chunks(r, 1))
    add("rt_simple_log_pairs", p, start + chunks(r, 2) + [("tick", T0 + 3)] + chunks(r[:4], 4))
    r = []
    for i in range(9):
        r += [nested(m32, "web-annotated", i), nested(m32, "web", i)]
    r += [nested(m32, "web-annotated", 9), nested(m32, "web", 9), nested(m11, "web-annotated", 10), nested(m11, "web", 10)]
    for i in range(2):
        r += [nested(m180, "web-annotated", i + 11, lkey="msg"), nested(m180, "web", i + 11, lkey="msg")]
    for i in range(2):
        r += [nested(m180, "web-annotated", i + 13, pkey="pod_alias"), nested(m180, "web", i + 13, pkey="pod_alias")]
    r += [nested(m180, "x", 20, wrapper="log", lkey="logwrapper"), nested(m180, "x", 21, kube="pod_name", pkey="kubernetes")]
    p = base + [("print_status", "false"), ("log_field", "logwrapper|log"), ("name_field", "kubernetes|pod_name")]
    add("rt_nested_log", p, start + chunks(r, 1))
    r = []
    for i in range(4):
        r += [simple(m32, "stdout", i), simple(m32, "stderr", i)]
    r += [simple(m32, "stdout", 9), simple(m32, "stdout", 9), simple(m32, "stderr", 9), simple(m6, "stdout", 10), simple(m6, "stderr", 10)]
    add("rt_default_name_field", base + [("print_status", "false"), ("log_field", "log")], start + chunks(r, 1))
    # (the runtime test's records carry 463 bytes of strings each: two make a rate of 30.87, the third would make 46.3 and is dropped)
    def full(pod, i):
        return nested(m32, pod, i, pad=463 - 3 - 292 - len(pod))
    r = [full("web-annotated", i) for i in range(3)] + [full("web", i) for i in range(3)]
    add("rt_default_log_field", [("rate", "43"), ("window", "30"), ("interval", "3s"), ("name_field", "kubernetes|pod_name"), ("print_status", "false"),
                                 ("window_time_duration", "10s")], start + chunks(r, 1))
    # ---- paths, names and loads
    small = [("rate", "10"), ("window", "5")]                    # 50 bytes a window
    keys = (rec(kv(("n", "a"), ("log", "x" * 20)), 1) + rec(kv((bv(b"n"), "a"), (bv(b"log"), "x" * 20)), 2) + rec(kv(("n", bv(b"a")), ("log", bv(b"y" * 20))), 3) +
            rec(kv(("n", "b"), ("n", "a"), ("log", "x" * 20), ("log", "x")), 4) + rec(kv((1, "a"), ("n", "c"), ("log", "x" * 60)), 5) +
            rec(kv(("n", "c"), ("log", "x" * 30)), 6) + rec(kv(("N", "c"), ("log", "x" * 30)), 7) + rec(kv(("nn", "c"), ("log", "x" * 30)), 8))
    add("keys_str_bin_duplicates", small + NL, start + [("chunk", keys)])
    others = [None, True, False, 7, -7, 0, f32(1.5), 2.5, ["a"], kv(("a", 1)), kv(), R(b"\xc7\x01\x05a"), sv(b""), bv(b"")]
    add("name_value_of_every_type", small + NL, start + [("chunk", b"".join(rec(kv(("n", v), ("log", "x" * 30)), i + 1) for i, v in enumerate(others)) * 2 + named(sv(b""), 51) + named(bv(b""), 50))])
    add("log_value_of_every_type", small + NL, start + [("chunk", b"".join(rec(kv(("n", "t%d" % i), ("log", v)), i + 1) for i, v in enumerate(others)) +
                                                         named("t0", 60) + named("t0", 50))])
    def deep(parts, leaf):
        o = leaf
        for k in reversed(parts):
            o = kv((k, o))
        return o
    for d in (1, 2, 20, 21):
        parts = ["k%d" % i for i in range(d)]
        body = lambda nm, n: R(synth.mp(kv(("N", deep(parts, nm)), ("L", deep(parts, "x" * n)))))
        data = b"".join(rec(body("a", 20), 1) + rec(body("a", 20), 2) + rec(body("a", 20), 3) + rec(body("b", 20), 4) for _ in range(1))
        add("path_depth_%d" % d, small + [("name_field", "|".join(["N"] + parts)), ("log_field", "|".join(["L"] + parts))], start + [("chunk", data)])
    # 21 parts behind the split's limit: the 21st entry is the rest of the line, separators and all
    parts = ["k%d" % i for i in range(22)]
    tailkey = "|".join(parts[19:])
    body = R(synth.mp(kv(("N", deep(parts[:19] + [tailkey], "a")), ("log", "x" * 30))))
    add("path_rest_of_the_line", small + [("name_field", "|".join(["N"] + parts)), ("log_field", "log")], start + [("chunk", rec(body, 1) * 3)])
    e = rec(kv(("a", kv(("b", "nm"), ("", kv(("b", "other"))))), ("", "top"), ("log", "x" * 30)), 1)
    for nm, f in (("empty_part_middle", "a||b"), ("empty_part_leading", "|a|b"), ("empty_part_trailing", "a|b|"), ("empty_part_two_trailing", "a|b||"),
                  ("empty_part_only", "|"), ("empty_field", "")):
        add("path_" + nm, small + [("name_field", f), ("log_field", "log")], start + [("chunk", e * 3)])
    add("path_log_empty_parts", small + [("name_field", "n"), ("log_field", "w||log|")], start + [("chunk", rec(kv(("n", "a"), ("w", kv(("log", "x" * 30)))), 1) * 3)])
    # nil, false and integer 0 where the path goes on: defined in the reference (a size of 0), not found
    add("path_through_nil_false_zero", small + [("name_field", "a|b"), ("log_field", "log")],
        start + [("chunk", b"".join(rec(kv(("a", v), ("log", "x" * 60)), i + 1) for i, v in enumerate([None, False, 0, kv(), kv(("b", "nm"))])))])
    big = "z" * 700
    nest = kv(("s8", str16(b"q" * 10)), ("s16", "r" * 300), ("s32", str32(b"t" * 5)), ("b", bv(b"u" * 7)), ("e", R(b"\xc7\x03\x05abc")), ("i", 12345), ("f", 2.5),
              ("arr", ["ab", ["cd", kv(("k", "ef"))], 5, None, bv(b"g")]), (bv(b"bk"), kv((3, "hi"))))
    add("load_nested_every_type", [("rate", "100"), ("window", "5"), ("name_field", "n"), ("log_field", "o")],
        start + [("chunk", rec(kv(("n", "a"), ("o", nest)), 1) * 2 + rec(kv(("n", "b"), ("o", kv(("x", big)))), 3))])
    add("load_whole_body", [("rate", "100"), ("window", "5"), ("name_field", "n")], start + [("chunk", rec(kv(("n", "a"), ("o", nest)), 1) * 2)])
    add("load_zero_leaves_timestamp", small + NL + [("interval", "1"), ("window_time_duration", "5")],
        [("now", T0), ("tick", T0), ("chunk", named("a", 10)), ("tick", T0 + 3), ("chunk", named("a", 0)), ("tick", T0 + 6), ("chunk", named("a", 0)),
         ("tick", T0 + 9), ("chunk", named("a", 45) + named("a", 10))])
    add("load_zero_creates_a_window", small + NL, start + [("chunk", named("a", 0) + named("a", 50) + named("a", 1))])
    # ---- the rate's edge
    edge = [("window", "30"), ("rate", "10")] + NL
    add("edge_sum_300_kept", edge, start + [("chunk", named("a", 100) + named("a", 200) + named("a", 1))])
    add("edge_sum_301_dropped", edge, start + [("chunk", named("a", 100) + named("a", 201) + named("a", 200))])
    add("edge_0001_in_binary64", [("window", "1000"), ("rate", "10")] + NL, start + [("chunk", named("a", 10001)), ("chunk", named("a", 1))])
    add("first_record_alone_too_large", small + NL, start + [("chunk", named("a", 51) + named("a", 50) + named("a", 1)), ("chunk", named("b", 500)), ("chunk", named("b", 5))])
    # ---- time
    tm = small + NL + [("interval", "1"), ("window_time_duration", "8")]
    add("small_after_dropped", tm, start + [("chunk", named("a", 40) + named("a", 20) + named("a", 30) + named("a", 10) + named("a", 1))])
    st = list(start) + [("chunk", named("a", 50))]
    for i in range(1, 8):
        st += [("tick", T0 + i), ("chunk", named("a", 10) + named("a", 45))]
    add("ticks_rotate_every_pane", tm, st)
    add("stale_deletion_then_the_name_again", tm, start + [("chunk", named("a", 50) + named("b", 5)), ("tick", T0 + 4), ("chunk", named("b", 5)), ("tick", T0 + 9),
                                                           ("chunk", named("a", 50)), ("tick", T0 + 13), ("tick", T0 + 20), ("now", T0 + 20), ("chunk", named("a", 50) + named("b", 50))])
    add("star_window_goes_stale", small + [("log_field", "log"), ("interval", "1"), ("window_time_duration", "8")],
        start + [("chunk", named("a", 30)), ("tick", T0 + 5), ("tick", T0 + 9), ("now", T0 + 9), ("chunk", named("a", 50) + named("b", 1)), ("tick", T0 + 30),
                 ("now", T0 + 31), ("chunk", named("a", 51) + named("a", 2))])
    add("star_window_untouched_goes_stale", small + [("interval", "1"), ("window_time_duration", "6")],
        start + [("tick", T0 + 6), ("tick", T0 + 7), ("now", T0 + 7), ("chunk", named("a", 3))])
    # ---- configuration
    # (a record of the default rate's size cannot be a fixture: the probes tell 1000 bytes a second from far more)
    probe = [("chunk", named("a", 1999) + named("a", 2))]
    for v in ("0", "-1", "1k", "1.5M", "x"):
        add("cfg_rate_%s" % v.strip(), [("rate", v), ("window", "2")] + NL, start + probe)
    for v in ("1", "2", "0", "3x", "x"):
        add("cfg_window_%s" % v, [("rate", "10"), ("window", v)] + NL, start + [("chunk", named("a", 20) + named("a", 10) + named("a", 20) + named("a", 1))])
    for v in ("0", "3s", "2m", "1x", "5ss", "0.5", "1h", "1d"):
        add("cfg_interval_%s" % v, [("rate", "10"), ("window", "3"), ("interval", v), ("window_time_duration", "7")] + NL,
            start + [("chunk", named("a", 20)), ("tick", T0 + 8), ("chunk", named("a", 20)), ("tick", T0 + 130), ("chunk", named("a", 30)), ("tick", T0 + 400),
                     ("chunk", named("a", 30))])
    add("cfg_duration_below_interval_times_window", [("rate", "10"), ("window", "4"), ("interval", "5"), ("window_time_duration", "3")] + NL,
        start + [("chunk", named("a", 20)), ("tick", T0 + 19), ("tick", T0 + 20), ("chunk", named("a", 40)), ("tick", T0 + 21), ("tick", T0 + 41), ("chunk", named("a", 40))])
    add("cfg_defaults", NL, start + [("chunk", named("a", 700) * 2)])
    add("cfg_names_without_case_and_ignored_ones", [("RATE", "10"), ("Window", "5"), ("print_status", "maybe"), ("nope", "1")] +
        [("NAME_FIELD", "n"), ("Log_Field", "log")], start + [("chunk", named("a", 30) * 3)])
    # ---- the chunk
    a, b = named("a", 30), named("b", 30)
    add("call_empty_chunk", small + NL, start + [("chunk", b""), ("chunk", a)])
    add("call_group_markers_all_kept", small + NL, start + [("chunk", a + GROUP_START + b + GROUP_END)])
    add("call_group_markers_with_a_drop", small + NL, start + [("chunk", a + GROUP_START + a + b + GROUP_END + a)])
    add("call_cut_record", small + NL, start + [("chunk", a + a + b + named("b", 30)[:-4])])
    add("call_cut_record_all_kept", small + NL, start + [("chunk", a + b + named("b", 1)[:-4])])
    add("call_garbage_reserved_byte", small + NL, start + [("chunk", a + a + b"\xc1\xff" + b)])
    add("call_non_map_body", small + NL, start + [("chunk", a + a + synth.mp([[synth.ext_ts(3), {}], "text"]) + b)])
    add("call_non_canonical_events", small + NL,
        start + [("chunk", (synth.mp([1700000000, kv(("n", "a"), ("log", "x" * 30))]) + synth.mp([1700000000.25, kv(("n", "a"), ("log", "x" * 30))]) +
                            rec(R(b"\xde\x00\x02" + b"\xd9\x01n" + b"\xd9\x01a" + b"\xda\x00\x03log" + b"\xdb\x00\x00\x00\x05xxxxx"), 3) +
                            synth.mp([[synth.ext_ts(7, 8), R(b"\xde\x00\x01\xd9\x01m\xd0\x05")], kv(("n", "a"), ("log", "x" * 15))]) + named("a", 1)))])
    add("call_all_dropped", small + NL, start + [("chunk", named("a", 100) + named("b", 100))])
    add("call_exempt_between_throttled", small + NL, start + [("chunk", a + rec(kv(("log", "x" * 99)), 2) + a + rec(kv(("n", "a")), 3) + b + named("a", 1))])
    # ---- names with a NUL byte: the reference stores the window under the cut name and looks it up by the whole one
    add("nul_in_name_alone", small + NL, start + [("chunk", named(sv(b"a\0b"), 30) * 3)])
    add("nul_in_name_beside_its_prefix", small + NL, start + [("chunk", named("a", 20) + named(sv(b"a\0b"), 30) + named("a", 20) + named(sv(b"a\0b"), 30) + named("a", 20))])
    return c


def plain(n, first=0):
    return [rec(kv(("i", first + i)), 1 + i) for i in range(n)]


def throttle_cases():
    c = []

    def add(name, props, steps):
        c.append((name, [tuple(p) for p in props], list(steps)))

    def ch(n, first=0):
        return ("chunk", b"".join(plain(n, first)))
    # ---- tests/runtime/filter_throttle.c: rate 1.4, window 1 (read as 5), interval 3s; 17 records, a tick between pushes
    p = [("rate", "1.4"), ("window", "1"), ("interval", "3s"), ("print_status", "true")]
    st = [("tick", T0)]
    for i in range(17):
        st += [ch(1, i)] + ([("tick", T0 + 3 * (i // 4 + 1))] if i % 4 == 3 else [])
    add("rt_throttle", p, st)
    add("rt_throttle_one_call", p, [("tick", T0), ch(17)])
    add("before_the_first_tick", [("rate", "2"), ("window", "3")], [ch(4), ch(4), ("tick", T0), ch(8), ("tick", T0 + 1), ch(3)])
    for k, props, n in ((0, [("rate", "2"), ("window", "2")], 5), (1, [("rate", "2"), ("window", "4")], 5), ("n_minus_1", [("rate", "2"), ("window", "5")], 10),
                        ("n", [("rate", "2"), ("window", "5")], 9), ("over_n", [("rate", "3"), ("window", "5")], 4)):
        pre = [("tick", T0), ch(4)] if k == 0 else [("tick", T0)] + ([ch(7)] if k == 1 else [])
        add("k_%s" % k, props, pre + [ch(n, 100)])
    add("ticks_with_a_repeated_timestamp", [("rate", "2"), ("window", "3")], [("tick", T0), ch(3), ("tick", T0), ch(3), ("tick", T0 + 1), ("tick", T0 + 1), ch(9), ("tick", T0), ch(2)])
    st = [("tick", T0)]
    for i in range(1, 9):
        st += [ch(5, 10 * i), ("tick", T0 + i)]
    add("window_wraps", [("rate", "3"), ("window", "3")], st + [ch(20)])
    for v in ("0.5", "1", "1.5", "2.5", "x", "-3"):
        add("cfg_rate_%s" % v, [("rate", v), ("window", "2")], [("tick", T0), ch(4), ("tick", T0 + 1), ch(4), ("tick", T0 + 2), ch(4)])
    for v in ("1", "0", "2", "x"):
        add("cfg_window_%s" % v, [("rate", "2"), ("window", v)], [("tick", T0), ch(12), ("tick", T0 + 1), ch(12)])
    for v in ("3s", "5ss", "1x", "0"):
        add("cfg_interval_%s" % v, [("rate", "2"), ("interval", v)], [("tick", T0), ch(12)])
    add("cfg_defaults", [], [("tick", T0), ch(7), ("tick", T0 + 1), ch(2)])
    a = plain(3)
    add("call_empty_chunk", [("rate", "2"), ("window", "2")], [("tick", T0), ("chunk", b""), ch(5)])
    add("call_group_markers", [("rate", "2"), ("window", "2")], [("tick", T0), ("chunk", a[0] + GROUP_START + a[1] + GROUP_END + a[2]), ("chunk", GROUP_START + a[0] + a[1] + GROUP_END + a[2])])
    add("call_cut_record", [("rate", "2"), ("window", "2")], [("tick", T0), ("chunk", a[0] + a[1] + a[2][:-2]), ("chunk", b"".join(plain(6)) + a[0][:-1])])
    add("call_garbage_and_non_map_body", [("rate", "2"), ("window", "2")], [("tick", T0), ("chunk", a[0] + b"\xc1" + a[1]), ("chunk", b"".join(plain(5)) + synth.mp([[synth.ext_ts(3), {}], "text"]) + a[0])])
    add("call_non_canonical_events", [("rate", "2"), ("window", "2")],
        [("tick", T0), ("chunk", synth.mp([1700000000, kv(("a", 1))]) + synth.mp([1700000000.25, kv(("a", 2))]) + rec(R(b"\xde\x00\x01\xa1a\xd0\x03"), 3) * 4)])
    return c


def admit_chunk(loads, name="a"):
    return b"".join(named(name, n, 1 + i) for i, n in enumerate(loads))


def fuzz_round(seed):
    """(props, steps): names and sizes drawn so that a round holds kept, dropped and exempt records"""
    rnd = random.Random(seed)
    window = rnd.choice([2, 5, 30])
    rate = rnd.choice([20, 100, 1000])
    props = [("rate", str(rate)), ("window", str(window)), ("interval", "1"), ("window_time_duration", str(rnd.choice([3, 40])))] + NL
    names = ["n%d" % i for i in range(rnd.choice([1, 3, 40, 300]))] + ["hot"]
    cap = rate * window
    steps, t = [("now", T0), ("tick", T0)], T0
    for _ in range(rnd.randint(2, 5)):
        recs = []
        for i in range(rnd.choice([1, 63, 64, 65, 300, 1500])):
            x = rnd.random()
            if x < 0.1:
                recs.append(rec(kv(("log", "x" * 5)), i) if rnd.random() < 0.5 else rec(kv(("n", rnd.choice([None, 5, ["a"]])), ("log", "x")), i))
            else:
                nm = "hot" if rnd.random() < 0.5 else rnd.choice(names)
                recs.append(named(nm, rnd.choice([0, 1, cap // 7, cap // 3, cap, cap + 1, 3 * cap]), i))
        steps.append(("chunk", b"".join(recs)))
        if rnd.random() < 0.7:
            t += rnd.randint(1, 4)
            steps += [("tick", t), ("now", t)]
    return props, steps
