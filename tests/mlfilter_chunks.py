"""The record builders, multiline parser definitions and deterministic chunks of the filter_multiline tests and of
tools/gen_mlfilter_golden.py, kept apart so that the chunks can be built and looked at without a device."""
import synth
from rtag_chunks import GROUP_END, GROUP_START, R, kv, rec  # noqa: F401

OFF = [("buffer", "off")]

# [MULTILINE_PARSER] definitions: name, type, negate, match string (endswith / equal), rules (from_states, regex, to_state)
CONT = dict(name="cont", type="regex", negate=0, match="", rules=[("start_state", r"/^\d{4}-\d\d-\d\d/", "cont"), ("cont", r"/^\s+/", "cont")])
# a rule that leads back to a start rule: the group is flushed behind the line that matches it (try_flushing_buffer)
BLOCK = dict(name="block", type="regex", negate=0, match="", rules=[("start_state", r"/^BEGIN/", "body"), ("body", r"/^\s/", "body"),
                                                                   ("body", r"/^END/", "start_state")])
EMPTYCONT = dict(name="emptycont", type="regex", negate=0, match="", rules=[("start_state", r"/^S/", "c"), ("c", r"/^$|^\+/", "c")])
# a start rule that matches an empty text: the empty group it opens is not flushed by the next start (flb_ml_rule.c:408-410)
EMPTYSTART = dict(name="emptystart", type="regex", negate=0, match="", rules=[("start_state", r"/^$|^S/", "c"), ("c", r"/^\+/", "c")])
EW = dict(name="ew", type="endswith", negate=0, match=";", rules=[])
EWN = dict(name="ewn", type="endswith", negate=1, match="\\", rules=[])
EQ = dict(name="eq", type="equal", negate=0, match="END", rules=[])
EQN = dict(name="eqn", type="equal", negate=1, match="...", rules=[])
PARSERS = {p["name"]: p for p in (CONT, BLOCK, EMPTYCONT, EMPTYSTART, EW, EWN, EQ, EQN)}


def props(parser, key="log", extra=()):
    return [("multiline.parser", parser), ("multiline.key_content", key)] + OFF + list(extra)


def logrec(text, i=0, **other):
    return rec(kv(("log", text), *other.items()), 1700000000 + i, i + 1)


def cont_text(i, kind, width=0):
    """kind: s start, c continuation, a a line nobody takes"""
    pad = "x" * width
    if kind == "s":
        return "2024-03-%02d 10:00:00 ERROR request %d failed %s" % (i % 28 + 1, i, pad)
    if kind == "c":
        return "    at com.example.Handler.run(Handler.java:%d) %s" % (i, pad)
    return "plain line %d %s" % (i, pad)


def mixed(n, seed=0):
    """n records for the `cont` parser, every item class and rule outcome in turn (from 2 records on: a start, a continuation, a line
    nobody takes, a record without the key, a record whose key is no STR); other entries of several types and positions of the key"""
    out = []
    for i in range(n):
        s = (i + seed) % 11
        t = 1700000000 + i
        if s in (0, 5):
            body = kv(("stream", "stdout"), ("log", cont_text(i, "s", i % 40)), ("n", i))
        elif s in (1, 2, 6, 7):
            body = kv(("log", cont_text(i, "c", (i * 7) % 90))) if s != 2 else kv(("log", cont_text(i, "c")), ("k", [1, {"a": None}]), ("f", 1.5))
        elif s == 3:
            body = kv(("a", R(b"\xd3" + (i % 100).to_bytes(8, "big"))), ("log", cont_text(i, "a")))
        elif s == 4:
            body = kv(("msg", "no key here %d" % i), ("b", R(b"\xdb\x00\x00\x00\x02hi")))
        elif s == 8:
            body = kv(("log", i), ("log", cont_text(i, "s")), ("z", True))
        elif s == 9:
            body = kv(("log", ""))
        else:
            body = kv(("log", R(b"\xc4\x03bin")), ("other", "x"))
        out.append(rec(body, t, i % 1000))
    return b"".join(out)


def one_group(n, width=20):
    return b"".join(logrec(cont_text(i, "s" if i == 0 else "c", width), i) for i in range(n))


def all_alone(n):
    return b"".join(logrec(cont_text(i, "s"), i, n=i) for i in range(n))


def group_of_bytes(total, nrec=3):
    """one group of the `cont` parser whose concatenation is exactly `total` bytes"""
    head = "2024-03-01 "
    if total <= len(head):
        raise ValueError(total)
    if total < len(head) + 2 * (nrec - 1) + 1 or nrec == 1:
        return logrec(head + "y" * (total - len(head))), 1
    rest = total - len(head) - 1 - (nrec - 1)            # a '\n' in front of every continuation
    per = rest // (nrec - 1)
    parts = [head + "y"] + [" " + "z" * (per - 1) for _ in range(nrec - 2)]
    parts.append(" " + "w" * (rest - per * (nrec - 2) - 1))
    assert sum(len(p) for p in parts) + nrec - 1 == total, (total, nrec)
    return b"".join(logrec(p, i) for i, p in enumerate(parts)), nrec


def wide_map(nentries, pos):
    """a first record of `nentries` entries with the content entry at index pos"""
    items = [("k%02d" % j, j) for j in range(nentries - 1)]
    items.insert(pos, ("log", "2024-03-01 wide"))
    return rec(kv(*items), 1700000000, 1) + logrec("  cont of wide", 1)


JAVA_TRACE = ["Jul 09, 2015 3:23:29 PM com.google.devtools.search.cloud.feeder.MakeLog: RuntimeException: Run from this message!",
              "  at com.my.app.Object.do$a1(MakeLog.java:50)", "  at java.lang.Thing.call(Thing.java:10)",
              "Caused by: com.example.myproject.MyProjectServletException", "  at com.my.app.Object.do$a1(MakeLog.java:51)", "  ... 27 common frames omitted",
              "nested exception is:", "java.lang.IllegalStateException: state", "\tat a.b.C.d(C.java:1)", "plain line"]
GO_TRACE = ["panic: my panic", "", "goroutine 4 [running]:", "panic(0x45cb40, 0x47ad70)",
            "\t/usr/local/go/src/runtime/panic.go:542 +0x46c fp=0xc42003f7b8 sp=0xc42003f710 pc=0x422f7c", "main.main()", "\tfoo.go:6 +0x39", "done"]
PYTHON_TRACE = ["Traceback (most recent call last):", '  File "/base/data/app.py", line 1535, in __call__', "    rv = self.handle_exception(request, response, e)",
                '  File "/base/app.py", line 5, in run', "    raise Exception('x')", "Exception: ('spam', 'eggs')", "after the trace"]
RUBY_TRACE = ["examble.rb:18:in `thrower': An error has occurred. (RuntimeError)", "\tfrom examble.rb:14:in `caller'", "\tfrom examble.rb:10:in `helper'", "plain"]
# the records flb_test_multiline_unbuffered (tests/runtime/filter_multiline.c) pushes; the test's own time of 0 takes the wall clock in the
# reference, so the recording gives them a time
REF_UNBUFFERED = ["panic: my panic", "\n", "goroutine 4 [running]:", "panic(0x45cb40, 0x47ad70)",
                  "  /usr/local/go/src/runtime/panic.go:542 +0x46c fp=0xc42003f7b8 sp=0xc42003f710 pc=0x422f7c", "main.main.func1(0xc420024120)"]
REF_UNBUFFERED_EXPECT = dict(records=6, pattern="panic", pattern_index=0)       # one record per push: "no concatenation"
