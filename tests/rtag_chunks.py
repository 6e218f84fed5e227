"""The record builders of the filter_rewrite_tag tests and of tools/gen_rtag_golden.py, kept apart so that the chunks can be built and
looked at without a device: hand-built events, the fixed pattern list of the device tests (patterns without the regex corners the
walkers count), the 1-rule and 16-rule configurations and the mixed chunk they run on."""
import struct

import synth

R = synth.Raw
GROUP_START = synth.mp([[R(b"\xd7\x00\xff\xff\xff\xff\x00\x00\x00\x00"), synth.KV([("g", 1)])], synth.KV([("r", 1)])])
GROUP_END = synth.mp([[R(b"\xd7\x00\xff\xff\xff\xfe\x00\x00\x00\x00"), {}], {}])


def rec(body, sec=1, nsec=0, meta=None):
    return synth.mp([[synth.ext_ts(sec, nsec), meta if meta is not None else {}], body])


def kv(*items):
    return synth.KV(list(items))


def f32(v):
    return R(b"\xca" + struct.pack(">f", v))


def f64bits(b):
    return R(b"\xcb" + struct.pack(">Q", b))


# ---- the device tests' configurations
P1 = [("Rule", "$log ^.*error.*$ err.$TAG false")]
# 16 rules of 8 template parts each: every part kind, keys and sub-keys of several lengths, keep alternating by rule; a third of
# mixed_records' rows match one of them
P16 = [("Rule", "$k%d ^never(%d)$ n%d.$TAG.$TAG[0].$1.$k%d.x.$0 %s" % (i, i, i, i, "true" if i % 2 else "false")) for i in range(6)] + [
    ("Rule", "$level ^(warn|error)$ lv.$1.$TAG[1].$level.$m['n'].$0.- true"),
    ("Rule", "$m['l'][1] ^([a-z]+)-(\\d+)$ sub.$1.$2.$TAG[0].$m['l'][1].$9.z false"),
    ("Rule", "$log ^.*(?<what>error|fatal).*$ $TAG.$1.$log.$TAG[2].$missing.$size.e true"),
    ("Rule", "user ^u(\\d)(\\d)?$ u.$1.$2.$TAG.$user.$TAG[9].q false"),
] + [("Rule", "$z%d ^(a)(b)?$ z%d.$1.$2.$TAG.$0.$z%d.y %s" % (i, i, i, "false" if i % 2 else "true")) for i in range(6)]
assert len(P16) == 16


def mixed_records(n):
    """shapes in turn, so that the lanes of a wave take different paths; about a third of them match a rule of P1 / P16"""
    out = []
    for i in range(n):
        s = i % 9
        if s == 0:
            body = kv(("log", "an error in line %d %s" % (i, "x" * (i % 37))), ("size", i * 31 - 7), ("stream", "stderr"))
        elif s == 1:
            body = {"log": "line %d %s" % (i, "had an error" if i % 2 else "is fine"), "stream": "stdout"}
        elif s == 2:
            body = kv(("level", "warn" if i % 2 else "info"), ("m", kv(("n", -i), ("l", [0, "ab-%d" % i if i % 4 == 0 else "ab_%d" % i, 2]))))
        elif s == 3:
            body = kv(("user", "u%d" % (i % 100)), ("user", 7 if i % 4 == 0 else ("u%d" if i % 4 == 1 else "v%d") % (i % 10)), ("log", 5))
        elif s == 4:
            body = kv(("m", kv(("l", ["x", "ABC-%d" % i]))), ("log", R(b"\xc4\x05error")))
        elif s == 5:
            body = kv(("log", "café error, fatal € %d" % i), ("size", 2.5 + i))
        elif s == 6:
            body = {}
        elif s == 7:
            body = kv((R(b"\xc4\x03log"), "an error"), ("z3", "ab" if i % 2 else "ba"), ("other", [1, 2, {"a": "b"}]))
        else:
            body = kv(("k", "v" * (i % 70)), ("log", "nothing to see " * (i % 5)))
        out.append(rec(body, 1700000000 + i, i))
    return b"".join(out)
