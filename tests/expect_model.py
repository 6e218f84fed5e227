"""CPU model of filter_expect (plugins/filter_expect/expect.c), restated on the msgpack walker of tests/modify_model.py: the config
map and context_create (:146-230, :580-632), the five rules in order with the first failure ending the record (rule_apply :275-396),
the messages the plugin logs, and one call under each action (:398-564) -- warn and exit never touch the chunk, result_key rebuilds
every record with {result_key: bool} in front of the body's own entries.  The model is the yardstick of tests/test_expect_*.py and
does not use the product."""
import struct

import checklist_model as clm
import modify_model as mm
import typeconv_model as tcm

MAX_RULES, MAX_TABLE_BYTES, MAX_RESULT_KEY = 64, 32768, 65535
WARN, EXIT, RESULT_KEY = 0, 1, 2
ACTIONS = ("warn", "exit", "result_key")
# rule kinds; ACTION is the rule an `action` property leaves in the list: it passes always and takes a rule number
KEY_EXISTS, KEY_NOT_EXISTS, KEY_VAL_NULL, KEY_VAL_NOT_NULL, KEY_VAL_EQ, ACTION = 0, 1, 2, 3, 4, 5
RULE_NAMES = ("key_exists", "key_not_exists", "key_val_is_null", "key_val_is_not_null", "key_val_eq", "action")
# failure kinds
NOT_FOUND, EXISTS, WRONG_TYPE, DIFFERENT = 1, 2, 3, 4
# value types (ra_value_type_to_str :254-273; a BIN is none of its five)
VT_NONE, VT_BOOL, VT_INT, VT_FLOAT, VT_STRING, VT_NULL, VT_BINARY = range(7)
VT_TEXT = ("", "boolean", "integer", "float / double", "string", "null", "UNKNOWN")


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def split_string(s):
    """flb_slist_split_string(list, s, ' ', 1) (src/flb_slist.c:223-313): the first run of bytes that are no spaces, then -- behind the
    spaces that follow -- the rest of the line as it is"""
    i, n = 0, len(s)
    while i < n and s[i] == 0x20:
        i += 1
    if i == n:
        return []
    j = s.find(b" ", i)
    if j < 0:
        return [s[i:]]
    out = [s[i:j]]
    k = j
    while k < n and s[k] == 0x20:
        k += 1
    if k < n:
        out.append(s[k:])
    return out


class Rule:
    def __init__(self, no, kind, value, ra, expect=None):
        self.no, self.kind, self.value, self.ra, self.expect = no, kind, value, ra, expect


class Config:
    pass


def _accessor(text):
    try:
        return tcm.accessor(text)
    except tcm.Skip:
        raise ValueError("the record accessor refuses %r" % text)


def parse(props):
    """the configuration; ValueError where the filter does not start or create refuses"""
    c = Config()
    c.action, c.result_key, c.rules = WARN, b"matched", []
    seen = set()
    items = []
    for name, val in props:
        name, val = _b(name).lower().decode(), _b(val).split(b"\0")[0]
        if b"${" in val:                                      # the engine would translate it when the property is set
            raise ValueError("environment variables are not translated")
        if name in ("action", "result_key"):                  # no FLB_CONFIG_MAP_MULT: set twice fails the check of the properties
            if name in seen:
                raise ValueError("%s is set more than once" % name)
            seen.add(name)
        elif name not in RULE_NAMES[:5]:
            raise ValueError("unknown property %s" % name)
        items.append((name, val))
    for name, val in items:
        if name == "action":
            if val.lower().decode("latin-1") not in ACTIONS:
                raise ValueError("unexpected action %r" % val)
            c.action = ACTIONS.index(val.lower().decode())
        elif name == "result_key":
            c.result_key = val
    if len(c.result_key) > MAX_RESULT_KEY:
        raise ValueError("result_key too long")
    for name, val in items:
        if name == "result_key":
            continue
        no = len(c.rules)
        if name == "action":
            c.rules.append(Rule(no, ACTION, val, None))       # (one of three words; whatever it finds, nobody looks at it)
        elif name == "key_val_eq":
            tok = split_string(val)
            if not tok:                                       # the reference takes the first and last entry of an empty list
                raise ValueError("key_val_eq without a value")
            c.rules.append(Rule(no, KEY_VAL_EQ, val, _accessor(tok[0]), tok[-1]))
        else:
            c.rules.append(Rule(no, RULE_NAMES.index(name), val, _accessor(val)))
    if len(c.rules) > MAX_RULES:
        raise ValueError("too many rules")
    if table_bytes(c) > MAX_TABLE_BYTES:
        raise ValueError("table too large")
    return c


def pad4(x):
    return (x + 3) // 4 * 4


def table_bytes(c):
    """the LDS table of expect.hpp"""
    n = 16 + pad4(len(mm.pack_str_hdr(len(c.result_key))) + len(c.result_key))
    for r in c.rules:
        n += 32
        if r.ra:
            key, subs = r.ra
            n += pad4(len(key)) + 8 * len(subs) + sum(pad4(len(x)) for k, x in subs if k == "s")
        if r.expect is not None:
            n += pad4(len(r.expect))
    return n


def describe(c):
    """the text flbgpu_expect_parse_check writes"""
    out = ["action=%s" % ACTIONS[c.action], "result_key=%s" % c.result_key.hex()]
    for r in c.rules:
        if r.ra is None:
            k = "-"
        else:
            k = "K" + r.ra[0].hex() + "".join("[%d]" % x if kind == "i" else "." + x.hex() for kind, x in r.ra[1])
        out.append("#%d:%s:%s%s" % (r.no, RULE_NAMES[r.kind], k, ":E" + r.expect.hex() if r.expect is not None else ""))
    return ";".join(out)


def vtype(o):
    """msgpack_object_to_ra_value (src/flb_ra_key.c:31-105): VT_NONE where it answers -1"""
    return {"bool": VT_BOOL, "uint": VT_INT, "int": VT_INT, "f32": VT_FLOAT, "f64": VT_FLOAT, "str": VT_STRING, "map": VT_BOOL, "bin": VT_BINARY,
            "nil": VT_NULL}.get(o.t, VT_NONE)


class Failure:
    """one failing record: its span in the input, the rule that failed with its number, how it failed, and the value it met"""
    def __init__(self, off, length, rule, kind, vt, val_off, val_len):
        self.off, self.len, self.rule, self.kind, self.vt, self.val_off, self.val_len = off, length, rule, kind, vt, val_off, val_len

    def entry(self):
        return (self.off, self.len, self.rule.no, self.kind, self.vt, self.val_off, self.val_len)


def failure_text(f, data):
    """the message flb_plg_error gets, up to and including "Record content:\\n" """
    r, v = f.rule, f.rule.value
    head = b"exception on rule #%d " % r.no
    if r.kind == KEY_EXISTS:
        return head + b"'key_exists', key '%s' not found. Record content:\n" % v
    if r.kind == KEY_NOT_EXISTS:
        return head + b"'key_not_exists', key '%s' exists. Record content:\n" % v
    if f.kind == NOT_FOUND:                                    # key_val_eq says 'key_val_is_null' here too (:366-373)
        name = b"key_val_is_not_null" if r.kind == KEY_VAL_NOT_NULL else b"key_val_is_null"
        return head + b"'%s', key '%s' not found. Record content:\n" % (name, v)
    if f.kind == WRONG_TYPE:
        return head + b"'%s', key '%s' contains a value type '%s'. Record content:\n" % (RULE_NAMES[r.kind].encode(), v, VT_TEXT[f.vt].encode())
    val = data[f.val_off:f.val_off + f.val_len].split(b"\0")[0]                  # printed with %s
    return head + b"'key_val_eq', key value '%s' is different than expected: '%s'. Record content:\n" % (val, r.expect)


def rule_apply(cfg, body, off, length):
    """rule_apply (:275-396): None, or the Failure of the first rule that fails"""
    for r in cfg.rules:
        o = clm.ra_value(r.ra, body)
        vt = vtype(o) if o is not None else VT_NONE
        if vt == VT_NONE:
            o = None
        val = (o.pay, len(o.v)) if vt == VT_STRING else (0, 0)

        def fail(kind):
            return Failure(off, length, r, kind, vt, *val)
        if r.kind == KEY_EXISTS:
            if o is None:
                return fail(NOT_FOUND)
        elif r.kind == KEY_NOT_EXISTS:
            if o is not None:
                return fail(EXISTS)
        elif r.kind in (KEY_VAL_NULL, KEY_VAL_NOT_NULL):
            if o is None:
                return fail(NOT_FOUND)
            if (vt == VT_NULL) != (r.kind == KEY_VAL_NULL):
                return fail(WRONG_TYPE)
        elif r.kind == KEY_VAL_EQ:
            if o is None:
                return fail(NOT_FOUND)
            # flb_sds_cmp: the lengths, then strncmp, which stops at a NUL the two share
            if vt == VT_STRING and (len(o.v) != len(r.expect) or o.v.split(b"\0")[0] != r.expect.split(b"\0")[0]):
                return fail(DIFFERENT)
    return None


class Model:
    """cb_expect_filter over a chunk: filter(data) -> (MODIFIED|NOTOUCH, bytes|None); counts() as flbgpu_filter_last_counts; counters()
    as flbgpu_expect_counters (since the model was created); failures: the last call's, in record order; exit_status: what
    config->exit_status_code reads after the call (0 or 255)"""
    MODIFIED, NOTOUCH = 1, 2

    def __init__(self, props):
        self.cfg = parse(props)
        self.stats = [0, 0, 0, 0]                 # records checked, records failed, exit requests, size/emit mismatches (none here)
        self.failures, self.exit_status = [], 0
        self.n_in = self.n_out = 0

    def texts(self, data):
        return [failure_text(f, bytes(data)) for f in self.failures]

    def filter(self, data):
        data, cfg = bytes(data), self.cfg
        self.failures, self.exit_status = [], 0
        out, p, n, n_out, clean = bytearray(), 0, 0, 0, True
        while p < len(data):
            try:
                end, skip, sec, nsec, meta, body = mm.decode_event(data, p)
            except mm.Bad:
                clean = mm.clean_cut(data, p)
                break
            start, p = p, end
            if skip:
                # a group marker goes out raw under result_key; any other negative time the decoder itself steps over
                if cfg.action == RESULT_KEY and sec in (-1, -2):      # (get_record_type reads the seconds alone)
                    out += data[start:end]
                continue
            n += 1
            f = rule_apply(cfg, body, start, end - start)
            self.stats[0] += 1
            if f is not None:
                self.failures.append(f)
                self.stats[1] += 1
                if cfg.action == EXIT:
                    self.exit_status = 255
                    self.stats[2] += 1
                    break
            if cfg.action == RESULT_KEY and 0 <= sec <= 0xffffffff and 0 <= nsec < 1000000000:
                # (a time the EventTime cannot hold: set_timestamp's answer is overwritten by the next decoder call, the record is gone)
                ents = [mm.canon(k) + mm.canon(v) for k, v in body.v]
                out += (b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + (mm.canon(meta) if meta is not None else b"\x80") + b"\xdf" +
                        struct.pack(">I", len(ents) + 1) + mm.pack_str_hdr(len(cfg.result_key)) + cfg.result_key + (b"\xc2" if f else b"\xc3") +
                        b"".join(ents))
                n_out += 1
        self.n_in = n
        if cfg.action == RESULT_KEY and clean:
            self.n_out = n_out
            return self.MODIFIED, bytes(out)
        self.n_out = n
        return self.NOTOUCH, None

    def counts(self):
        return self.n_in, self.n_out

    def counters(self):
        return tuple(self.stats)
