"""filter_multiline, mode parser with buffer off (plugins/filter_multiline/ml.c:839-909), restated in plain Python: the decoder loop
feeds every record to flb_ml_append_event (src/multiline/flb_ml.c:763-875, process_append / package_content :207-501, the rule state
machine src/multiline/flb_ml_rule.c:245-436, flb_ml_group_cat src/multiline/flb_ml_group.c:87-122) on one stream with one parser,
flb_ml_flush_pending_now flushes what is open (flb_ml_flush_stream_group :1590-1800).  The searches are the oracle's own orx_search
(rtag_model.Rx).  What the device does not reproduce is said by Refused (the configuration) and by filter() answering -1 (a record
with a non-empty metadata map, a record with an empty text that starts a group)."""
import struct

import modify_model as mm
from rtag_model import Rx

MODIFIED, NOTOUCH = 1, 2
REGEX, ENDSWITH, EQ = 0, 1, 2
BUILTIN = {
    "java": [("start_state, java_start_exception", r"/(.)(?:Exception|Error|Throwable|V8 errors stack trace)[:\r\n]/", "java_after_exception"),
             ("java_after_exception", r"/^[\t ]*nested exception is:[\t ]*/", "java_start_exception"),
             ("java_after_exception", r"/^[\r\n]*$/", "java_after_exception"),
             ("java_after_exception, java", r"/^[\t ]+(?:eval )?at /", "java"),
             ("java_after_exception, java", r"/^[\t ]+--- End of inner exception stack trace ---$/", "java"),
             ("java_after_exception, java", r"/^--- End of stack trace from previous (?x:)location where exception was thrown ---$/", "java"),
             ("java_after_exception, java", r"/^[\t ]*(?:Caused by|Suppressed):/", "java_after_exception"),
             ("java_after_exception, java", r"/^[\t ]*... \d+ (?:more|common frames omitted)/", "java")],
    "go": [("start_state", r"/\bpanic: /", "go_after_panic"), ("start_state", r"/http: panic serving/", "go_goroutine"),
           ("go_after_panic", r"/^$/", "go_goroutine"), ("go_after_panic, go_after_signal, go_frame_1", r"/^$/", "go_goroutine"),
           ("go_after_panic", r"/^\[signal /", "go_after_signal"), ("go_goroutine", r"/^goroutine \d+ \[[^\]]+\]:$/", "go_frame_1"),
           ("go_frame_1", r"/^(?:[^\s.:]+\.)*[^\s.():]+\(|^created by /", "go_frame_2"), ("go_frame_2", r"/^\s/", "go_frame_1")],
    "python": [("start_state", r"/^Traceback \(most recent call last\):$/", "python"), ("python", r"/^[\t ]+File /", "python_code"),
               ("python_code", r"/[^\t ]/", "python"), ("python", r"/^(?:[^\s.():]+\.)*[^\s.():]+:/", "start_state")],
    "ruby": [("start_state, ruby_start_exception", r"/^.+:\d+:in\s+.*/", "ruby_after_exception"),
             ("ruby_after_exception, ruby", r"/^\s+from\s+.*:\d+:in\s+.*/", "ruby")],
}
DEFAULT_LIMIT = 2 * 1024 * 1024
KNOWN = ("debug_flush", "buffer", "mode", "flush_ms", "multiline.parser", "multiline.key_content", "emitter_name", "emitter_storage.type", "emitter_mem_buf_limit")


class Refused(Exception):
    pass


def utils_bool(v):
    """flb_utils_bool: 1, 0, or -1 for anything else"""
    v = v.lower()
    return 1 if v in ("true", "on", "yes") else 0 if v in ("false", "off", "no") else -1


class Parser:
    """a [MULTILINE_PARSER]: dict(name, type, negate, match, rules[(from_states, regex, to_state)]) or a built-in name"""

    def __init__(self, d, limit=DEFAULT_LIMIT):
        self.name = d["name"]
        self.type = {"regex": REGEX, "endswith": ENDSWITH, "equal": EQ}[d["type"]]
        self.negate = bool(d["negate"])
        self.match = d["match"].encode() if isinstance(d["match"], str) else bytes(d["match"])
        self.limit = limit
        self.key_content = d.get("key_content")
        self.rules = []
        for fr, rx, to in d["rules"]:
            states = [s.strip(" ") for s in fr.split(",")]
            self.rules.append(dict(frm=[s for s in states if s], rx=Rx.get(rx.encode()), to=to or None, start="start_state" in states))
        for r in self.rules:          # flb_ml_rule_init: to_state_map in rule order
            r["map"] = [j for j, q in enumerate(self.rules) if r["to"] is not None and r["to"] in q["frm"]]


def builtin(name, limit=DEFAULT_LIMIT):
    return Parser(dict(name=name, type="regex", negate=0, match="", rules=BUILTIN[name], key_content="log"), limit)


def parse(props, parsers):
    """-> dict(parser=name, key=bytes | None): what create keeps; Refused says why it does not start.  parsers: names defined"""
    cfg = dict(buffer=1, mode="parser", names=[], key=None)
    for k, v in props:
        kl = k.lower()
        if kl not in KNOWN:
            raise Refused("unknown property '%s'" % k)
        if kl == "buffer":
            cfg["buffer"] = utils_bool(v)
        elif kl == "mode":
            cfg["mode"] = v.lower()
        elif kl == "multiline.parser":
            cfg["names"] += [t.strip(" ") for t in v.split(",") if t.strip(" ")]
        elif kl == "multiline.key_content":
            cfg["key"] = v.encode()
    if cfg["mode"] not in ("parser", "partial_message"):
        raise Refused("'Mode' must be 'partial_message' or 'parser'")
    if cfg["mode"] == "partial_message":
        raise Refused("mode partial_message is not built")
    if cfg["buffer"] != 0:
        raise Refused("buffered mode is not built: say 'buffer off'")
    if not cfg["names"]:
        raise Refused("mode parser requires at least one 'multiline.parser'")
    if len(cfg["names"]) > 1:
        raise Refused("more than one multiline parser is not built")
    name = cfg["names"][0]
    if name in ("docker", "cri"):
        raise Refused("a multiline parser with a parser in front ('%s') is not built" % name)
    if name not in parsers and name not in BUILTIN:
        raise Refused("multiline parser '%s' is not defined" % name)
    return dict(parser=name, key=cfg["key"])


def describe(cfg, parser=None):
    """the line flbgpu_multiline_parse_check writes; parser: the Parser behind the name, None for a custom name without a definition"""
    if parser is None and cfg["parser"] in BUILTIN:
        parser = builtin(cfg["parser"])
    key = cfg["key"] if cfg["key"] is not None else (parser.key_content.encode() if parser is not None and parser.key_content else None)
    text = "parser=%s key_content=%s" % (cfg["parser"], key.decode() if key is not None else "(none)")
    if parser is not None:
        text += " type=%s rules=%d buffer_limit=%d" % (("regex", "endswith", "equal")[parser.type], len(parser.rules), parser.limit)
    return text


class Model:
    """cb_ml_filter over consecutive chunks: filter(data) -> (MODIFIED | NOTOUCH | -1, bytes | None); counts() as
    flbgpu_filter_last_counts, counters() as flbgpu_multiline_counters, state() as flbgpu_multiline_state"""

    def __init__(self, props, parsers=None, limit=DEFAULT_LIMIT, mutate=None, hand_back_empty_start=True):
        defs = {n: (p if isinstance(p, Parser) else Parser(p, limit)) for n, p in (parsers or {}).items()}
        self.cfg = parse(props, defs)
        n = self.cfg["parser"]
        self.p = defs[n] if n in defs else builtin(n, limit)
        key = self.cfg["key"]
        if key is None and self.p.key_content:
            key = self.p.key_content.encode()
        self.key = key
        self.buf, self.ctx, self.time, self.trunc, self.state = b"", [], (0, 0), False, None
        self.tot = [0, 0, 0, 0]
        self.n_in = self.n_out = 0
        self.mutate = mutate or ""
        self.hand_back_empty_start = hand_back_empty_start     # False: what the reference does with such a call
        self.empty_start = False
        self.out = []

    # ---- the stream group
    def _flush(self):
        body = None
        if self.ctx:
            m = self.ctx[0]
            if self.buf:
                ln = len(self.key)
                parts = [mm.pack_hdr(len(m.v), 0x80, 0xde, 0xdf) if self.mutate != "map32" else b"\xdf" + struct.pack(">I", len(m.v))]
                for k, v in m.v:
                    hit = False
                    if k.t == "str" and len(k.v) == ln:
                        kc = self.key + b"\0" * (ln + 1)
                        hit = True
                        for i in range(ln):            # strncmp(k, key_content, len)
                            if k.v[i] != kc[i]:
                                hit = False
                                break
                            if k.v[i] == 0:
                                break
                    if hit:
                        parts += [mm.canon(k), mm.pack_str_hdr(len(self.buf)), self.buf]
                        ln = len(self.buf)             # the loop's `len` now holds the buffer's length
                    else:
                        parts += [mm.canon(k), mm.canon(v)]
                body = b"".join(parts)
            else:
                body = mm.canon(m)
            self.ctx = []
        elif self.buf:
            body = b"\x81" + mm.pack_str_hdr(len(self.key)) + self.key + mm.pack_str_hdr(len(self.buf)) + self.buf
        if body is not None:
            meta = b"\xdf\x00\x00\x00\x01\xb3multiline_truncated\xc3" if self.trunc else b"\xdf\x00\x00\x00\x00"
            sec, nsec = self.time if self.mutate != "calltime" else self.call_time
            self.out.append(b"\x92\x92\xd7\x00" + struct.pack(">II", sec & 0xffffffff, nsec) + meta + body)
        self.buf, self.trunc = b"", False

    def _register(self, tm, m):
        self.time = tm
        self.ctx.append(m)

    def _cat(self, data):
        """flb_ml_group_cat: True when truncated"""
        L, t = self.p.limit, False
        if L > 0:
            if len(self.buf) >= L:
                self.trunc = True
                return True
            if len(data) > L - len(self.buf):
                data, t, self.trunc = data[:L - len(self.buf)], True, True
        self.buf += data
        return t

    def _try_flushing(self):
        r = self.state
        if r is None or any(self.p.rules[j]["start"] for j in self.p.rules[r]["map"]):
            if self.buf:
                self._flush()

    def _rule_process(self, val, tm, m):
        """flb_ml_rule_process: 0, -1 (nobody takes it) or 'trunc'"""
        rule = None
        R = self.p.rules
        if self.state is not None:
            for j in R[self.state]["map"]:
                if R[j]["start"]:
                    continue
                if R[j]["rx"].search(val) is not None:
                    if self.buf and self.buf[-1:] != b"\n" and self.mutate != "nosep":
                        self.buf += b"\n"
                    if not val:
                        self.buf += b"\n"
                    elif self._cat(val):
                        self._flush()
                        self.state = None
                        return "trunc"
                    rule = j
                    break
        if rule is None:
            for j, r in enumerate(R):
                if r["start"] and r["rx"].search(val) is not None:
                    rule = j
                    break
            if rule is not None:
                if self.buf:
                    self._flush()
                self.state = rule
                if not val:
                    self.empty_start = True
                if self._cat(val):
                    return "trunc"
                self._register(tm, m)
        if rule is None:
            return -1
        self.state = rule
        self._try_flushing()
        return 0

    def _content(self, m):
        """get_key_id: the first entry whose key is a STR equal to key_content and whose value is a STR"""
        if self.key is None:
            return None
        hit = None
        for k, v in m.v:
            if k.t == "str" and v.t == "str" and k.v == self.key:
                hit = v.v
                if self.mutate != "lastkey":
                    break
        return hit

    def _append(self, tm, m):
        """flb_ml_append_object -> 0 (OK) or 'trunc'"""
        val, p, done = self._content(m), self.p, False
        if val is not None:
            if p.type == REGEX:
                r = self._rule_process(val, tm, m)
                if r == "trunc":
                    return "trunc"
                if r == 0:
                    if not self.ctx:
                        self._register(tm, m)
                    done = True
            elif p.type == EQ or len(p.match) <= len(val):
                hit = (val == p.match) if p.type == EQ else val.endswith(p.match)
                if not self.ctx:
                    self._register(tm, m)
                self.buf += val
                if hit != p.negate:
                    self._flush()
                done = True
        if not done:
            self._flush()
            if self.mutate == "reset":
                self.state = None
            self._register(tm, m)
            self._flush()
        return 0

    def filter(self, data, call_time=(0, 0)):
        data = bytes(data)
        self.call_time = call_time
        # a record with a non-empty metadata map is handed back: the call fails and changes nothing
        p, recs = 0, []
        while p < len(data):
            try:
                end, skip, sec, nsec, meta, body = mm.decode_event(data, p)
            except mm.Bad:
                break
            p = end
            if skip:
                continue
            if meta is not None and meta.v:
                self.tot[2] += 1
                self.n_in = self.n_out = 0
                return -1, None
            recs.append(((sec, nsec), body))
        self.out = []
        before = (self.buf, list(self.ctx), self.time, self.trunc, self.state, list(self.tot))
        self.empty_start = False
        for tm, body in recs:
            if self._append(tm, body) == "trunc":
                self.tot[1] += 1
            else:
                self.tot[0] += 1
        self._flush()
        if self.empty_start and self.hand_back_empty_start:
            # a record with an empty text started a group: handed back like metadata, the stream stays where it was
            self.buf, self.ctx, self.time, self.trunc, self.state, self.tot = before
            self.tot[2] += 1
            self.n_in = self.n_out = 0
            self.out = []
            return -1, None
        self.n_in, self.n_out = len(recs), len(self.out)
        if not self.out:
            return NOTOUCH, None
        return MODIFIED, b"".join(self.out)

    def counts(self):
        return self.n_in, self.n_out

    def counters(self):
        return tuple(self.tot)

    def state_of(self):
        return -1 if self.state is None else self.state

    def classes(self, data):
        """what the records of a chunk are, without moving the model: the set of item classes and rule outcomes (coverage floors)"""
        import copy
        m = copy.copy(self)
        m.ctx, m.tot = list(self.ctx), list(self.tot)
        seen, p = set(), 0
        data = bytes(data)
        while p < len(data):
            try:
                end, skip, sec, nsec, meta, body = mm.decode_event(data, p)
            except mm.Bad:
                break
            p = end
            if skip:
                continue
            if meta is not None and meta.v:
                seen.add("metadata")
                continue
            val = m._content(body)
            if val is None or (m.p.type == ENDSWITH and len(m.p.match) > len(val)):
                seen.add("not_processed")
                m._append((sec, nsec), body)
                continue
            seen.add("rules")
            if m.p.type == REGEX:
                before, nbuf = m.state, len(m.buf)
                hit_cont = before is not None and any(not m.p.rules[j]["start"] and m.p.rules[j]["rx"].search(val) is not None for j in m.p.rules[before]["map"])
                hit_start = any(r["start"] and r["rx"].search(val) is not None for r in m.p.rules)
                seen.add("continuation" if hit_cont else "start" if hit_start else "alone")
            m._append((sec, nsec), body)
        return seen
