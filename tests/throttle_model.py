"""CPU model of filter_throttle_size (plugins/filter_throttle_size/throttle_size.c, size_window.c, size_window.h) and filter_throttle
(plugins/filter_throttle/throttle.c, window.c), restated on the msgpack walker of tests/modify_model.py: the configuration as
configure / the config map read it, the nested name and log lookups (first key that is STR or BIN with the part's bytes), the
recursive payload size, the windows with their greedy admission, one trip of each ticker, and one cb_filter call (the kept records'
own bytes; NOTOUCH when all were kept).  What strtod, strtoul, atof and atoi accept is libc's, asked through ctypes.  The model is
the yardstick of tests/test_throttle_*.py and does not use the product.

Where the model follows the product and not the reference: a name holding a NUL byte is the name, whole; a path that
continues through a value that is no map finds nothing."""
import ctypes
import time

import modify_model as mm

MODIFIED, NOTOUCH = 1, 2             # FLB_FILTER_MODIFIED, FLB_FILTER_NOTOUCH
_libc = ctypes.CDLL(None)
_libc.strtod.restype = ctypes.c_double
_libc.strtod.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
_libc.strtoul.restype = ctypes.c_ulong
_libc.strtoul.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
_libc.atoi.restype = ctypes.c_int
_libc.atoi.argtypes = [ctypes.c_char_p]


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def strtod(s):
    """(value, the bytes behind what was read)"""
    s = _b(s)
    buf = ctypes.create_string_buffer(s)
    end = ctypes.c_char_p()
    v = _libc.strtod(buf, ctypes.byref(end))
    return v, end.value


def size_to_bytes(s):
    """flb_utils_size_to_bytes (src/flb_utils.c:527-608)"""
    s = _b(s)
    if s.lower() == b"false":
        return 0
    if not s:
        return -1
    val = strtod(s)[0]
    plen = 0
    for i in range(len(s) - 1, 0, -1):
        if 0x30 <= s[i] <= 0x39:
            break
        plen += 1

    def i64(v):
        return -1 if (v != v or v >= 2.0 ** 63 or v <= -2.0 ** 63) else int(v)
    if plen == 0:
        return i64(val)
    if plen > 2:
        return -1
    tmp = s[len(s) - plen:].upper()
    if plen == 2 and tmp[1:2] != b"B":
        return -1
    if tmp[0:1] == b"K":
        return -1 if (val >= 9223372036854775.0 or val <= -9223372036854774.0) else i64(val * 1000)
    if tmp[0:1] == b"M":
        return -1 if (val >= 9223372036854 or val <= -9223372036853) else i64(val * 1000000)
    if tmp[0:1] == b"G":
        return -1 if (val >= 9223372036 or val <= -9223372035) else i64(val * 1000000000)
    return -1


def utils_split(line, sep=b"|", max_split=20):
    """flb_utils_split (src/flb_utils.c:321-457, no quotes)"""
    line = _b(line)
    out, i, n = [], 0, len(line)
    while i < n:
        t = i
        while t < n and line[t:t + 1] == sep:
            t += 1
        e = line.find(sep, t)
        if e < 0:
            e = n
        out.append(line[t:e])
        i = e + 1
        if len(out) >= max_split and i < n:
            out.append(line[i:])
            break
    return out


SUFFIX = {b"": 1, b"s": 1, b"m": 60, b"h": 3600, b"d": 86400}


def _prop(props, name):
    for k, v in props:
        if _b(k).lower() == name:
            return _b(v)
    return None


class Refused(Exception):
    pass


class SizeConfig:
    def __init__(self, props):
        self.rate, self.window, self.interval, self.duration = 1048576.0, 5, 1, 60
        self.name_parts, self.log_parts = [], []
        s = _prop(props, b"rate")
        if s is not None:
            b = size_to_bytes(s)
            if b > 0:
                self.rate = float(b)
        s = _prop(props, b"window")
        if s is not None:
            val = float(_libc.strtoul(s, None, 10))
            if val > 1:
                if val > 65536:
                    raise Refused("window over 65536 panes")
                self.window = int(val)
        s = _prop(props, b"interval")
        if s is not None:
            self.interval = self.parse_duration(s, 1)
        s = _prop(props, b"log_field")
        if s is not None:
            self.log_parts = utils_split(s)
        s = _prop(props, b"name_field")
        if s is not None:
            self.name_parts = utils_split(s)
        s = _prop(props, b"window_time_duration")
        if s is not None:
            self.duration = self.parse_duration(s, 60)
        if self.interval * self.window > 2 ** 31 - 1:
            raise Refused("interval * window")
        if self.duration < self.interval * self.window:
            self.duration = self.interval * self.window
        if 8 + sum(8 + (len(p) + 3) // 4 * 4 for p in self.name_parts + self.log_parts) > 32768:
            raise Refused("path table")

    @staticmethod
    def parse_duration(text, default):
        """parse_duration (:478-499)"""
        s, rest = strtod(text)
        if 0 >= s or len(rest) > 1 or rest not in SUFFIX:
            return default
        s *= SUFFIX[rest]
        if not s < 2.0 ** 31:
            raise Refused("duration")
        return int(s)

    def describe(self):
        def path(parts):
            return "|".join(p.hex() for p in parts) if parts else "-"
        return "rate=%s;window=%d;interval=%d;duration=%d;name=%s;log=%s" % (g17(self.rate), self.window, self.interval, self.duration,
                                                                               path(self.name_parts), path(self.log_parts))


def g17(v):
    """printf("%.17g")"""
    return "%.17g" % v


def lookup(obj, parts):
    """get_value_of_msgpack_object_map (:287-305): None when not found"""
    for part in parts:
        if obj.t != "map":
            return None                     # (the reference reads it as a map: DESIGN 8)
        for k, v in obj.v:
            if k.t in ("str", "bin") and k.v == part:
                obj = v
                break
        else:
            return None
    return obj


def load_of(obj):
    """get_msgpack_object_size (:220-246)"""
    if obj.t in ("str", "bin"):
        return len(obj.v)
    if obj.t == "map":
        return sum(load_of(k) + load_of(v) for k, v in obj.v)
    if obj.t == "array":
        return sum(load_of(v) for v in obj.v)
    return 0


class SizeWindow:
    def __init__(self, size, now):
        self.size, self.total, self.head, self.tail, self.timestamp = size, 0, size - 1, 0, now
        self.panes = [[now, 0] for _ in range(size)]

    def add_new_pane(self, ts):
        tail_size = self.panes[self.tail][1]
        if self.size - 1 == self.head:
            self.head = -1
        self.head += 1
        self.panes[self.head] = [ts, 0]
        self.total = (self.total - tail_size) % 2 ** 64
        if self.size - 1 == self.tail:
            self.tail = -1
        self.tail += 1

    def add_load(self, load):
        self.panes[self.head][1] += load
        self.total += load
        if load:
            self.timestamp = self.panes[self.head][0]


def events(data):
    """the decoder's loop over a chunk: (start, end, skip, body) of every event up to the first one it refuses"""
    p = 0
    while p < len(data):
        try:
            end, skip, _sec, _nsec, _meta, body = mm.decode_event(data, p)
        except mm.Bad:
            return
        yield p, end, skip, body
        p = end


class ThrottleSize:
    def __init__(self, props, now=None):
        self.cfg = SizeConfig(props)
        self.now = now
        self.windows = {}
        self.n_in = self.n_kept = self.n_dropped = self.n_exempt = self.created = self.deleted = 0
        self.started = False
        if not self.cfg.name_parts:
            self.windows[b"*"] = SizeWindow(self.cfg.window, self._now())
            self.created = 1

    def _now(self):
        return self.now if self.now else int(time.time())

    def set_now(self, t):
        self.now = t
        if not self.started and not self.cfg.name_parts:
            self.windows[b"*"] = SizeWindow(self.cfg.window, self._now())

    def over(self, total):
        return float(total) / float(self.cfg.window) - self.cfg.rate > 0.001

    def record(self, body):
        """throttle_data_by_size (:308-433): 'keep', 'drop' or 'exempt'"""
        c = self.cfg
        if c.name_parts:
            nv = lookup(body, c.name_parts)
            if nv is None or nv.t not in ("str", "bin"):
                return "exempt"
            name = nv.v
        else:
            name = b"*"
        if c.log_parts:
            lv = lookup(body, c.log_parts)
            if lv is None:
                return "exempt"
            load = load_of(lv)
        else:
            load = load_of(body)
        if not name:
            # flb_hash_table_get and flb_hash_table_add refuse a key of no bytes: judged alone, every time, and nothing is stored
            return "drop" if self.over(load) else "exempt"
        w = self.windows.get(name)
        if w is None:
            if self.over(load):
                return "drop"
            w = self.windows[name] = SizeWindow(c.window, self._now())
            self.created += 1
            w.add_load(load)
            return "keep"
        if self.over(w.total + load):
            return "drop"
        w.add_load(load)
        return "keep"

    def filter(self, data):
        self.started = True
        out, n_in, n_out = bytearray(), 0, 0
        self.last = []
        for start, end, skip, body in events(data):
            if skip:
                continue
            n_in += 1
            v = self.record(body)
            self.last.append(v)
            self.n_exempt += v == "exempt"
            if v != "drop":
                out += data[start:end]
                n_out += 1
        self.n_in += n_in
        self.n_kept += n_out
        self.n_dropped += n_in - n_out
        if n_in == n_out:
            return NOTOUCH, None
        return MODIFIED, bytes(out)

    def tick(self, ts):
        """the ticker's loop body (:175-186)"""
        self.started = True
        ts = ts if ts else int(time.time())
        for w in self.windows.values():
            w.add_new_pane(ts)
        threshold = int(float(ts) - float(self.cfg.duration))
        for name in [n for n, w in self.windows.items() if threshold > w.timestamp]:
            del self.windows[name]
            self.deleted += 1

    def view(self):
        return {n: dict(total=w.total, timestamp=w.timestamp, head=w.head, panes=[tuple(p) for p in w.panes]) for n, w in self.windows.items()}

    def counters(self):
        return dict(records=self.n_in, kept=self.n_kept, dropped=self.n_dropped, exempt=self.n_exempt, live=len(self.windows),
                    created=self.created, deleted=self.deleted)


# ---------------------------------------------------------------- filter_throttle
def utils_bool(v):
    v = _b(v).lower()
    return 1 if v in (b"true", b"on", b"yes") else 0 if v in (b"false", b"off", b"no") else -1


class ThrottleConfig:
    def __init__(self, props):
        rate, window, interval = 1.0, 5, b"1"
        seen = set()
        for k, v in props:
            k, v = _b(k).lower(), _b(v)
            if b"${" in v or k not in (b"rate", b"window", b"print_status", b"interval") or k in seen:
                raise Refused(k)
            seen.add(k)
            if k == b"rate":
                rate = strtod(v)[0]
            elif k == b"window":
                window = _libc.atoi(v)
            elif k == b"print_status":
                if utils_bool(v) < 0:
                    raise Refused(k)
            else:
                interval = v
        self.rate = 1.0 if rate <= 1.0 else rate
        window &= 0xffffffff
        self.window = 5 if window <= 1 else window
        if self.window > 65536:
            raise Refused("window")
        s, rest = strtod(interval)
        if not (0 >= s or len(rest) > 1) and rest in SUFFIX:
            s *= SUFFIX[rest]
        if not -2.0 ** 31 - 1 < s < 2.0 ** 31:
            raise Refused("interval")
        self.interval = int(s)

    def describe(self):
        return "rate=%s;window=%d;interval=%d" % (g17(self.rate), self.window, self.interval)


class Throttle:
    def __init__(self, props):
        self.cfg = ThrottleConfig(props)
        self.size = self.cfg.window
        self.table = [[0, 0] for _ in range(self.size)]
        self.current_timestamp, self.total, self.max_index = 0, 0, -1
        self.n_in = self.n_kept = self.n_dropped = 0

    def window_add(self, ts, val):
        """window_add (window.c:69-97)"""
        self.current_timestamp = ts
        for p in self.table:
            if p[0] == ts:
                p[1] += val
                break
        else:
            if self.size - 1 == self.max_index:
                self.max_index = -1
            self.max_index += 1
            self.table[self.max_index] = [ts, val]
        self.total = sum(p[1] for p in self.table)

    def tick(self, ts):
        ts = ts if ts else int(time.time())
        self.window_add(ts, 0)
        self.current_timestamp = ts

    def filter(self, data):
        out, n_in, n_out = bytearray(), 0, 0
        for start, end, skip, _body in events(data):
            if skip:
                continue
            n_in += 1
            if self.total / float(self.size) >= self.cfg.rate:
                continue
            self.window_add(self.current_timestamp, 1)
            out += data[start:end]
            n_out += 1
        self.n_in += n_in
        self.n_kept += n_out
        self.n_dropped += n_in - n_out
        if n_in == n_out:
            return NOTOUCH, None
        return MODIFIED, bytes(out)


def replay(kind, case):
    """the steps of a recorded case through the model: [(ret, out)] per chunk step"""
    import base64
    m = (ThrottleSize if kind == "throttle_size" else Throttle)([tuple(p) for p in case["props"]])
    res = []
    for st in case["steps"]:
        if st[0] == "now":
            m.set_now(st[1])
        elif st[0] == "tick":
            m.tick(st[1])
        else:
            res.append(m.filter(base64.b64decode(st[1])))
    return m, res
