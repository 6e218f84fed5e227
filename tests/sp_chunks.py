"""Named cases for the stream processor's aggregation kernels (csrc/sp_kernels.inc, csrc/sp_select.inc and the host half csrc/sp.cpp):
every case sits on one edge of that code --

  staging       k_sp_extract's tiles: 1, 63, 64, 65 and 257 rows; a wave's rows whose running size (first-row alignment included) is
                exactly SP_TILE at row k and one byte more; a row longer than the tile (the direct path) at lane 0, in the middle and
                at lane 63, two of them in a row; a chunk whose last 16-byte load crosses its end; emptied rows; and all of it once
                more with a decimal string under the aggregated key (those rows leave the tile for k_sp_generic)
  keys          one chunk of duplicate keys, bin-typed keys, sub-keys to depth SP_MAX_SUB, a first entry that is no map before one that
                is, a duplicated GROUP BY key standing in for a missing one -- under pairs of queries that differ by a seventh distinct
                key (sp_walk against sp_lookup); every SP_MAX_* limit at its value, and one past it (refused at create)
  multiplicity  1 .. 65 536 string entries of one aggregated key / GROUP BY key in one record, bin-typed ones mixed in, also under a
                plain SELECT
  dictionary    growth of the group dictionary inside the stream processor (FLBGPU_L2M_INIT_CAP / FLBGPU_L2M_INIT_ARENA): 8 and 9
                groups, an arena filled exactly and one byte more, a key longer than four arenas, 1000 groups in one call, growth in
                the second chunk of a window, a second window, one wave of one / of 64 new groups, tuples that collide unless class
                bytes and terminators are honoured, a row split in two (the rows behind it must not count)
  values        sums whose every partial sum is exact in binary64 (so the comparison is on bytes): the smallest subnormal, limb shifts
                0 / 1 / 31, +-DBL_MAX cancelling, negative and zero totals, carries out of every touched digit; INT64_MIN / MAX, uint64
                above 2^63, wrapping integer sums, integers before / after a float, with and without a wrap ahead of the float (the
                reference's answer follows the arrival order, and so does the device's); MIN / MAX over mixed classes; numeric strings at the 19 / 20 byte boundary; record times of
                2^31 seconds and more
  grid          (built from the CU count of the launch) the second trip of k_sp_extract, k_sp_aggregate and k_sp_generic, the LDS
                combiner's spill, one slot every lane contends for, k_sp_normalize's second trip

A case is (SQL, str_conv, steps, env) where a step is a chunk for StreamTask.do, a (bytes, row offsets) pair for do_dev, or the timer;
check() says, from the bytes alone, that the case is on its edge; want() is the oracle's (oracle/osp.py) answer per step.  tests/test_sp_chunks.py runs the predicates on the CPU and
holds the oracle's answers against the reference binary and tests/golden/sp_edges_kat.json; tests/test_sp_edges_gpu.py runs the cases
on the device."""
import hashlib
import os
import re
import struct
import sys
from fractions import Fraction

import msgpack

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import osp

CSRC = os.path.join(os.path.dirname(HERE), "fluent-bit_amd", "csrc")
REFUSED = "refused"
GROUPS = ("staging", "keys", "multiplicity", "dictionary", "values", "grid")
NOMINAL_CUS = 256                          # the grid group on the CPU (the device test builds it from the launch's own count)
SELECT_GRID = (4096, 256)                  # launch_sp_select: at most 4096 blocks of 256 lanes
GENERIC_GRID = (4096, 64)                  # launch_sp_generic
NORMALIZE_GRID = (64, 256)                 # k_sp_normalize's launch in launch_sp_aggregate


def limits():
    """the constants of the device code, read from its sources (tests/test_sp_chunks.py::test_limits_are_those_of_the_device_code
    also pins the three launch shapes above)"""
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("dev.hpp", "sp_kernels.inc", "l2m_kernels.inc"))
    lim = {}
    for name in ("SP_TILE", "SP_BLOCK", "SP_FAST_KEYS", "SP_MAX_KEYS", "SP_MAX_GB", "SP_MAX_SRC", "SP_MAX_SUB", "SP_MAX_LEAF", "SP_MAX_OPS",
                 "L2M_AGG_SLOTS", "L2M_AGG_BLOCK", "L2M_NLIMB", "SP_SRC_MAX", "SP_A_LIMB"):
        m = re.search(r"constexpr int (?:[A-Z0-9_]+ = \d+, *\s*)*%s = (\d+)" % name, src)
        assert m, name
        lim[name] = int(m.group(1))
    m = re.search(r"constexpr int SP_SRC_ADD = SP_A_LIMB \+ (\d+);", src)
    lim["SP_SRC_ADD"] = lim["SP_A_LIMB"] + int(m.group(1))
    m = re.search(r"constexpr uint32_t SP_VT_MANY = (\d+);", src)
    lim["SP_VT_MANY"] = int(m.group(1))
    return lim


LIM = limits()
SP_TILE, SP_BLOCK = LIM["SP_TILE"], LIM["SP_BLOCK"]


# ------------------------------------------------------------------------------------------ bytes
def P(v):
    return msgpack.packb(v, use_bin_type=True)


def mp_map(pairs):
    """a map of already packed (key, value) pairs in the narrowest header"""
    n = len(pairs)
    hdr = bytes([0x80 | n]) if n < 16 else b"\xde" + struct.pack(">H", n) if n < 65536 else b"\xdf" + struct.pack(">I", n)
    return hdr + b"".join(k + v for k, v in pairs)


def rec(pairs, sec=1700000000, nsec=0):
    """[[time, {}], body]"""
    return b"\x92\x92\xd7\x00" + struct.pack(">II", sec, nsec) + b"\x80" + mp_map(pairs)


def body(d):
    return [(P(k), P(v)) for k, v in d.items()]


def offsets(rows, first=0):
    off = [first]
    for r in rows:
        off.append(off[-1] + len(r))
    return off


def one_object(b):
    """b is exactly one msgpack object"""
    u = msgpack.Unpacker(raw=True, strict_map_key=False)
    u.feed(b)
    try:
        u.unpack()
    except Exception:
        return False
    return u.tell() == len(b)


class Dev:
    """a chunk for do_dev: the bytes and the row offsets into them (rows may be empty; a row that is no msgpack object ends the chunk)"""

    def __init__(self, rows, first=0, tail=b""):
        self.rows = list(rows)
        self.off = offsets(self.rows, first)
        self.data = b"\0" * first + b"".join(self.rows) + tail

    def first_bad(self):
        return next((i for i, r in enumerate(self.rows) if r and not one_object(r)), None)

    def oracle_bytes(self):
        k = self.first_bad()
        return b"".join(self.rows if k is None else self.rows[:k])


TIMER = "timer"


def need(ok, *ctx):
    assert ok, ctx
    return True


class ExactTask(osp.Task):
    """osp.Task that also keeps every SUM / AVG as a Fraction (an integer-typed sum: the wrapped int64, which is what the reference
    converts when the first float arrives): `inexact` names the first float-typed sum whose binary64 value is not the exact one
    (then the reference's sequential additions and the device's one rounding of the exact sum may part), `f32_rounds` the packaged
    float SUMs that are no float32 numbers (what leaves is then blind below the rounding)"""
    _exact = {}
    inexact = None
    f32_rounds = []

    def _reset(self):
        osp.Task._reset(self)
        ExactTask._exact = {}

    def _package(self, now=(1, 0)):
        for node in self.order:
            for ki, ck in enumerate(self.q.keys):
                num = node["nums"][ki]
                if ck.func == osp.FLB_SP_SUM and num.type == "f" and abs(num.f64) != float("inf") and num.f64 == num.f64:
                    if osp._to_f32(num.f64) != num.f64:
                        ExactTask.f32_rounds.append(num.f64)
        return osp.Task._package(self, now)

    @staticmethod
    def _add(func, num, ival, dval):
        osp.Task._add(func, num, ival, dval)
        if func in (osp.FLB_SP_AVG, osp.FLB_SP_SUM):
            ex = ExactTask._exact
            if dval != dval or dval in (float("inf"), float("-inf")):
                ex[id(num)] = None
            elif num.type == "i":
                ex[id(num)] = Fraction(num.i64)
            elif ex.get(id(num), 0) is not None:
                ex[id(num)] = ex.get(id(num), 0) + Fraction(ival) + Fraction(dval)
                if Fraction(num.f64) != ex[id(num)] and ExactTask.inexact is None:
                    ExactTask.inexact = (num.f64, ex[id(num)])


class Case:
    def __init__(self, name, sql, steps, pred=None, str_conv=True, env=None, notes=None, ref=True):
        self.name, self.sql, self.steps, self.pred, self.str_conv = name, sql, list(steps), pred, str_conv
        self.env, self.notes, self.ref = dict(env or {}), dict(notes or {}), ref
        self._want = None

    def step_bytes(self, s):
        return s.oracle_bytes() if isinstance(s, Dev) else s

    def want(self):
        """per step (records, bytes) of do / do_dev, the bytes of the timer; REFUSED from the step the oracle refuses at"""
        if self._want is None:
            ExactTask.inexact, ExactTask.f32_rounds = None, []
            t = ExactTask(self.sql, str_conv=self.str_conv)
            res = []
            for s in self.steps:
                try:
                    res.append(t.timer() if s is TIMER else t.do(self.step_bytes(s)))
                except osp.Unsupported:
                    res.append(REFUSED)
                    break
            self._want, self.inexact, self.f32_rounds = res, ExactTask.inexact, ExactTask.f32_rounds
        return self._want

    def run(self, task):
        """the same steps on anything with do / timer (the reference binary, the oracle with other settings)"""
        return [task.timer() if s is TIMER else tuple(task.do(self.step_bytes(s))) for s in self.steps]

    def digest(self):
        h = hashlib.sha256()
        for s in self.steps:
            if isinstance(s, Dev):
                h.update(b"D" + struct.pack("<Q", len(s.data)) + s.data + b"".join(struct.pack("<Q", o) for o in s.off))
            elif s is TIMER:
                h.update(b"T")
            else:
                h.update(b"H" + struct.pack("<Q", len(s)) + s)
        w = self.want()
        ret = [x if x == REFUSED else x[0] if isinstance(x, tuple) else -1 for x in w]
        out = b"".join(b"R" if x == REFUSED else struct.pack("<Q", len(x[1])) + x[1] if isinstance(x, tuple) else struct.pack("<Q", len(x)) + x for x in w)
        return {"case": self.name, "chunk_sha256": h.hexdigest(), "ret": ret, "sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out)}

    def check(self):
        w = self.want()
        assert self.inexact is None, (self.name, "a float-typed sum is not exact in binary64", self.inexact)
        # a float SUM leaves as binary32: exact there too, or the case says what the rounding still shows
        assert not self.f32_rounds or self.notes.get("f32"), (self.name, "a float SUM is no float32 number", self.f32_rounds[:3])
        assert (REFUSED in w) == (self.notes.get("refused") is not None), (self.name, w[-1])
        if REFUSED in w:
            assert w.index(REFUSED) == self.notes["refused"], self.name
        if self.pred:
            self.pred(self)

    def rows_out(self, step=-1):
        w = self.want()[step]
        u = msgpack.Unpacker(raw=True, strict_map_key=False)
        u.feed(w[1] if isinstance(w, tuple) else w)
        return [r[1] for r in u]


# ------------------------------------------------------------------------------------------ staging
def tile_plan(off):
    """k_sp_extract's walk over a chunk's rows: per wave of 64 rows the batches [(first lane, rows, 'tile' | 'direct', staged bytes)]"""
    n = len(off) - 1
    plan = []
    for base in range(0, n, 64):
        cnt = min(64, n - base)
        lo, wave = 0, []
        while lo < cnt:
            g0 = off[base + lo]
            align = g0 & 15
            m = 0
            while lo + m < cnt and off[base + lo + m + 1] - g0 + align <= SP_TILE:
                m += 1
            if m == 0:
                wave.append((lo, 1, "direct", 0))
                lo += 1
            else:
                wave.append((lo, m, "tile", off[base + lo + m] - g0 + align))
                lo += m
        plan.append(wave)
    return plan


STAGE_SQL = "SELECT g, COUNT(*), SUM(v), MIN(v), MAX(v) FROM STREAM:s WINDOW TUMBLING (5 SECOND) GROUP BY g;"


def dec_row(i):
    """the rows of the `dec` staging cases whose aggregated value is a decimal string"""
    return i % 5 == 2 or i in (0, 64)


def stage_row(i, size=None, dec=False):
    """a record of `size` bytes (None: as short as it comes) whose GROUP BY key and aggregated key are its LAST entries, behind the
    padding; every row carries other values, so a row read through a wrong base gives a wrong answer.  dec: the values of the rows
    dec_row() names are strings with a decimal point (exact in binary: the sums stay exact)"""
    v = P("%d.5" % (i % 97)) if dec and dec_row(i) else P(i * 7 + 1)
    tailp = [(P("g"), P(i % 5)), (P("v"), v)]
    if size is None:
        return rec([(P("p"), P("x" * (i % 9)))] + tailp)
    fixed = len(rec([(P("p"), b"")] + tailp))
    for hdr, room, head in ((1, 31, lambda n: bytes([0xa0 | n])), (2, 255, lambda n: b"\xd9" + bytes([n])), (3, 65535, lambda n: b"\xda" + struct.pack(">H", n)),
                            (5, 2 ** 32 - 1, lambda n: b"\xdb" + struct.pack(">I", n))):
        n = size - fixed - hdr                                        # (a wider header than the string needs is msgpack all the same)
        if 0 <= n <= room:
            r = rec([(P("p"), head(n) + bytes([97 + i % 26]) * n)] + tailp)
            assert len(r) == size, (len(r), size)
            return r
    raise ValueError("no padding gives a row of %d bytes" % size)


def _stage_pred(expect):
    def pred(c):
        d = c.steps[0]
        plan = tile_plan(d.off)
        expect(c, d, plan)
        assert len(c.rows_out()) == len({i % 5 for i, r in enumerate(d.rows) if r}), c.name
    return pred


def staging_cases(dec=False):
    tag = "staging/dec/" if dec else "staging/"
    notes = {"deferred": dec}
    cs = []

    def add(name, dev, expect):
        cs.append(Case(tag + name, STAGE_SQL, [dev, TIMER], _stage_pred(expect), notes=dict(notes)))

    for n in (1, 63, 64, 65, 257):
        def expect(c, d, plan, n=n):
            assert len(plan) == (n + 63) // 64 and sum(m for w in plan for _, m, _, _ in w) == n and all(k == "tile" for w in plan for _, _, k, _ in w)
        add("rows/%d" % n, Dev([stage_row(i, dec=dec) for i in range(n)]), expect)
    # rows 0..k end exactly at the tile's last byte / one byte behind it
    for k in (1, 2, 63):
        for al in (0, 1, 15):
            for over in (0, 1):
                total = SP_TILE - al + over
                each = total // (k + 1)
                sizes = [each] * k + [total - each * k]
                rows = [stage_row(i, sizes[i] if i <= k else None, dec) for i in range(64)]
                def expect(c, d, plan, k=k, al=al, over=over):
                    lo, m, kind, staged = plan[0][0]
                    assert d.off[0] & 15 == al and d.off[k + 1] - d.off[0] + al == SP_TILE + over
                    assert (lo, kind) == (0, "tile") and (m, staged) == ((k + 1, SP_TILE) if not over else (k, staged)) and staged <= SP_TILE
                add("fit/k%d/a%d/%s" % (k, al, "over" if over else "exact"), Dev(rows, first=al), expect)
    for lane in (0, 31, 63):
        rows = [stage_row(i, SP_TILE + 1 + 40 * lane if i == lane else None, dec) for i in range(64)]
        def expect(c, d, plan, lane=lane):
            assert [b for b in plan[0] if b[2] == "direct"] == [(lane, 1, "direct", 0)]
        add("direct/lane%d" % lane, Dev(rows), expect)
    rows = [stage_row(i, SP_TILE + 16 * i if i in (20, 21) else None, dec) for i in range(64)]
    def expect(c, d, plan):
        assert [b[0] for b in plan[0] if b[2] == "direct"] == [20, 21]
    add("direct/two_in_a_row", Dev(rows), expect)
    # the chunk's last 16-byte load reaches past data + bytes: the last record's aggregated value is in those bytes
    for mod in (1, 8, 15):
        rows = [stage_row(i, dec=dec) for i in range(70)]
        grow = (mod - sum(len(r) for r in rows)) % 16
        rows[3] = stage_row(3, len(rows[3]) + grow + 16, dec)
        def expect(c, d, plan, mod=mod):
            assert len(d.data) % 16 == mod and d.off[-1] == len(d.data) and d.data[-4:] == b"v" + P(69 * 7 + 1)
            lo, m, kind, staged = plan[-1][-1]
            assert kind == "tile" and (d.off[-1] - staged) % 16 == 0 and staged % 16 != 0       # the last load starts aligned and is partial
        add("tail/mod%d" % mod, Dev(rows), expect)
    for where, empty in (("first", {0}), ("middle", {30, 31}), ("last", {66}), ("batch", set(range(64)))):
        rows = [b"" if i in empty else stage_row(i, dec=dec) for i in range(67)]
        def expect(c, d, plan, empty=empty):
            assert all(d.off[i] == d.off[i + 1] for i in empty) and sum(1 for r in d.rows if not r) == len(empty)
        add("empty/" + where, Dev(rows), expect)
    return cs


# ------------------------------------------------------------------------------------------ keys
def keys_chunk():
    sub = {"x": {"y": {"z": 9, "w": 1}}, "n": 4}
    recs = []
    for i in range(70):
        d = [("t", 1), ("a", i % 3), ("b", i % 2), ("c", i), ("d", 100 - i), ("e", i % 4), ("s", dict(sub, n=i))]
        p = body(dict(d))
        if i % 7 == 1:
            p.append((P("c"), P(1000)))                               # a duplicate of the aggregated key: the first value, twice
        if i % 7 == 2:
            p.insert(0, (P(b"c"), P(5)))                              # a bin-typed key of the same name, first: its value, once
        if i % 7 == 3:
            p = [x for x in p if x[0] != P("s")]
            p += [(P("s"), P(5)), (P("s"), P(sub))]                   # the first entry is no map: the sub-keys are ignored
        if i % 7 == 4:
            p = [x for x in p if x[0] != P("b")]
            p.append((P("a"), P(2)))                                  # {a, a} under GROUP BY a, b: found == 2, b = 0
        if i % 7 == 5:
            p = [x for x in p if x[0] != P("b")]                      # GROUP BY key missing: the record is dropped
        if i % 7 == 6:
            p.append((P(b"a"), P(7)))                                 # a bin-typed GROUP BY key behind the string one
        recs.append(rec(p, 1700000000 + i))
    return b"".join(recs)


def _limit_sql(what, n):
    """a query with exactly n of `what`"""
    ks = ["k%d" % i for i in range(16)]
    if what == "keys":          # 4 GROUP BY + 6 aggregated + (n - 10) WHERE operands
        return "SELECT COUNT(*), %s FROM STREAM:s WHERE %s GROUP BY k0, k1, k2, k3;" % (
            ", ".join("SUM(k%d)" % i for i in range(4, 10)), " AND ".join("k%d >= 0" % i for i in range(10, n)))
    if what == "gb":
        return "SELECT COUNT(*) FROM STREAM:s GROUP BY %s;" % ", ".join(ks[:n])
    if what == "src":
        return "SELECT %s FROM STREAM:s;" % ", ".join("SUM(k%d)" % i for i in range(n))
    if what == "sub":
        return "SELECT MAX(m%s) FROM STREAM:s;" % "".join("['l%d']" % i for i in range(n))
    if what == "leaf":          # a comparison is two leaves, a bare key one
        return "SELECT COUNT(*) FROM STREAM:s WHERE %s;" % " AND ".join(["k0 >= 0"] * (n // 2) + ["k1"] * (n % 2))
    if what == "ops":           # 8 comparisons + 7 ANDs, the rest NOTs in front of the whole (an even number: the identity)
        nots = n - 15
        return "SELECT COUNT(*) FROM STREAM:s WHERE %s%s;" % ("NOT " * nots, " AND ".join(["k0 >= 0"] * 7 + ["k1 < 0" if nots % 2 else "k1 >= 0"]))
    raise ValueError(what)


def keys_cases():
    lim = LIM
    cs = []
    chunk = keys_chunk()
    base = ("SELECT a, b, COUNT(*), SUM(c), MIN(d), MAX(s['x']['y']['z']) FROM STREAM:s WHERE e >= 0%s GROUP BY a, b;",
            "SELECT a, COUNT(c), AVG(c), MAX(d), MIN(s['n']) FROM STREAM:s WINDOW TUMBLING (5 SECOND) WHERE NOT e < 0%s GROUP BY a, s['x']['y']['z'];")
    for qi, q in enumerate(base):
        for nk, extra in ((6, ""), (7, " AND t = 1")):
            def pred(c, nk=nk):
                assert len(osp_keys(c.sql)) == nk and (nk <= lim["SP_FAST_KEYS"]) == (nk == 6)
            cs.append(Case("keys/q%d/%dkeys" % (qi, nk), q % extra, [chunk, TIMER], pred, notes={"pair": "keys/q%d" % qi}))
    m = {"l0": {"l1": {"l2": 77, "l3": {"deep": 1}}}}
    for i, (what, name) in enumerate((("keys", "SP_MAX_KEYS"), ("gb", "SP_MAX_GB"), ("src", "SP_MAX_SRC"), ("sub", "SP_MAX_SUB"), ("leaf", "SP_MAX_LEAF"), ("ops", "SP_MAX_OPS"))):
        n = lim[name]
        recs = [rec(body(dict({"k%d" % j: (r + j) % 3 for j in range(16)}, m=dict(m, r=r))), 1700000000 + r) for r in range(66)]
        def pred(c, what=what, n=n):
            assert len(c.rows_out(0)) >= 1 and c.want()[0][0] > 0
            if what == "keys":
                assert len(osp_keys(c.sql)) == n and len(osp_keys(c.notes["over"])) == n + 1
        cs.append(Case("keys/limit/" + what, _limit_sql(what, n), [b"".join(recs), TIMER], pred, notes={"over": _limit_sql(what, n + 1), "limit": name}))
    return cs


LIMIT_OF = {"keys": "SP_MAX_KEYS", "gb": "SP_MAX_GB", "src": "SP_MAX_SRC", "sub": "SP_MAX_SUB", "leaf": "SP_MAX_LEAF", "ops": "SP_MAX_OPS"}


def plan_counts(sql):
    """what the device's plan holds of a query, counted from the oracle's parse: distinct keys, GROUP BY columns, distinct aggregated
    keys, the deepest sub-key path, and the leaves and ops of the condition as csrc/sp.cpp emits them (a comparison: two leaves and
    an op; a bare key or value: a leaf and an op; NOT, AND, OR: an op; parentheses: nothing)"""
    q = osp.parse(sql)
    refs = [(g[0], tuple(g[1] or ())) for g in q.gb_keys] + [(k.name, tuple(k.subkeys or ())) for k in q.keys if k.name is not None]
    n = {"keys": len(osp_keys(sql)), "gb": len(q.gb_keys), "src": len({(k.name, tuple(k.subkeys or ())) for k in q.keys if k.func and k.name is not None}),
         "sub": max([len(r[1]) for r in refs] + [0]), "leaf": 0, "ops": 0}

    def walk(c):
        if c is None:
            return
        assert c.a[0] == "op", c.a
        op, l, r = c.a[1], c.a[2], c.a[3]
        if op == "PAR":
            walk(l)
        elif op == "NOT":
            walk(l)
            n["ops"] += 1
        elif op in ("AND", "OR") and l is not None and r is not None and l.a[0] == "op" and r.a[0] == "op":
            walk(l)
            walk(r)
            n["ops"] += 1
        elif op == "OR":                                              # the truth value of one key / value
            n["leaf"] += 1
            n["ops"] += 1
        else:
            n["leaf"] += 2
            n["ops"] += 1
    walk(q.cond)
    return n


def osp_keys(sql):
    """the distinct key references of a query, as the device's plan counts them"""
    q = osp.parse(sql)
    seen = set()
    for g in q.gb_keys:
        seen.add((g[0], tuple(g[1] or ())))
    for k in q.keys:
        if k.name is not None:
            seen.add((k.name, tuple(k.subkeys or ())))

    def walk(c):
        if not isinstance(c, osp.Cond):
            return
        if c.a[0] == "key":
            seen.add((c.a[1], tuple(c.a[2] or ())))
        for x in c.a[1:]:
            walk(x)
    walk(q.cond)
    return seen


# ------------------------------------------------------------------------------------------ multiplicity
MULTS = (1, 2, 63, 64, 65, 255, 256, 65535, 65536)
MULT_AGG = "SELECT COUNT(b), SUM(b), AVG(b), MIN(b), MAX(b) FROM STREAM:s;"
MULT_GB = "SELECT g, h, COUNT(*), SUM(v) FROM STREAM:s GROUP BY g, h;"


def multiplicity_cases():
    cs = []
    for n in MULTS:
        one = rec([(P("b"), P(3))] * n) + rec([(P("b"), P(5))], 1700000001)
        def pred(c, n=n):
            assert c.steps[0].count(b"\xa1b\x03") == n
            r = c.rows_out(0)
            if b"SUM(b)" in r[0]:
                assert r[0][b"SUM(b)"] == 3 * n + 5
            else:
                assert len(r) == 2 and len(c.want()[0][1]) > 3 * n                         # a pair per entry
        cs.append(Case("multiplicity/agg/%d" % n, MULT_AGG, [one], pred))
        cs.append(Case("multiplicity/select/%d" % n, "SELECT b FROM STREAM:s;", [one], pred))
        flt = rec([(P("b"), P(0.5))] * n) + rec([(P("b"), P(2))], 1700000001)
        cs.append(Case("multiplicity/float/%d" % n, MULT_AGG, [flt], lambda c, n=n: need(c.steps[0].count(b"\xa1b\xcb") == n, c.name)))
        # a GROUP BY key n times and its neighbour h missing: the entries of g stand in for h from two on
        gb = rec([(P("g"), P(1))] * n + [(P("v"), P(2))]) + rec(body({"g": 2, "h": 3, "v": 4}), 1700000001)
        def predg(c, n=n):
            assert c.steps[0].count(b"\xa1g\x01") == n and len(c.rows_out(0)) == (2 if n >= 2 else 1)
        cs.append(Case("multiplicity/groupby/%d" % n, MULT_GB, [gb], predg))
    for n in (62, 63, 65536):
        # bin-typed entries of the name mixed in: the value is the first entry's whatever its type, the count is the string entries'
        mixed = rec([(P(b"b"), P(7))] + [(P("b"), P(3)), (P(b"b"), P(4))] * n)
        def pred(c, n=n):
            assert c.rows_out(0)[0][b"SUM(b)"] == 7 * n
        cs.append(Case("multiplicity/bin_mixed/%d" % n, MULT_AGG, [mixed], pred))
        cs.append(Case("multiplicity/bin_mixed/select/%d" % n, "SELECT b FROM STREAM:s;", [mixed], None))
    # 65 536 bin-typed entries of a GROUP BY key and one string entry: found = 65 537, and one string entry of the aggregated key
    many = rec([(P("g"), P(1))] + [(P(b"g"), P(9))] * 65536 + [(P(b"v"), P(1))] * 65536 + [(P("v"), P(2))])
    def pred(c):
        assert c.rows_out(0) == [{b"g": 1, b"h": 0, b"COUNT(*)": 1, b"SUM(v)": 1}]
    cs.append(Case("multiplicity/bin_only_65536", MULT_GB, [many], pred))
    return cs


# ------------------------------------------------------------------------------------------ dictionary
DICT_ENV = {"FLBGPU_L2M_INIT_CAP": "16", "FLBGPU_L2M_INIT_ARENA": "64"}
DICT_SQL = "SELECT k, COUNT(*), SUM(v) FROM STREAM:s WINDOW TUMBLING (5 SECOND) GROUP BY k;"
DICT_SQL2 = "SELECT k, j, COUNT(*), SUM(v) FROM STREAM:s WINDOW TUMBLING (5 SECOND) GROUP BY k, j;"


def krec(k, v, i=0, **more):
    return rec(body(dict({"k": k, "v": v}, **more)), 1700000000 + i)


def key_bytes(vals):
    """arena bytes of a tuple of GROUP BY values: a class byte each, then 8 bytes or the string and its NUL; padded to 8"""
    n = sum(1 + (len(v.encode()) + 1 if isinstance(v, str) else 8) for v in vals)
    return (n + 7) & ~7


def dictionary_cases():
    cs = []

    def add(name, sql, steps, grows, groups_after=None, pred=None, **kw):
        """grows: (lowest, highest or None) number of dictionary growths after each do / do_dev step, cumulative"""
        cs.append(Case("dictionary/" + name, sql, steps, pred, env=DICT_ENV, notes=dict(grows=grows, **kw)))

    for n in (8, 9):
        ch = b"".join(krec("k%d" % (i % n), i, i) for i in range(3 * n))
        def pred(c, n=n):
            assert n * key_bytes(["k0"]) == 64 + 8 * (n - 8) and len(c.rows_out()) == n
        add("groups/%d" % n, DICT_SQL, [ch, TIMER], [(0, 0) if n == 8 else (1, None)], pred=pred)
    for ln, g in ((62, (0, 0)), (63, (1, None))):
        def pred(c, ln=ln):
            assert key_bytes(["x" * ln]) == (64 if ln == 62 else 72)
        add("arena/%s" % ("exact" if ln == 62 else "one_more"), DICT_SQL, [krec("x" * ln, 1) + krec("x" * ln, 2, 1), TIMER], [g], pred=pred)
    add("long_key", DICT_SQL, [krec("L" * 300, 1) + krec("s", 2, 1) + krec("L" * 300, 3, 2), TIMER], [(3, None)],
        pred=lambda c: need(key_bytes(["L" * 300]) > 4 * 64, c.name))
    ch = b"".join(krec(i % 1000, i, i) for i in range(1300))
    add("groups/1000", DICT_SQL, [ch, TIMER], [(7, None)], pred=lambda c: need(len(c.rows_out()) == 1000, c.name))
    first = b"".join(krec("a%d" % (i % 4), i, i) for i in range(40))
    second = b"".join(krec("b%d" % (i % 40), 1000 + i, i) for i in range(80)) + b"".join(krec("a%d" % (i % 4), 7, i) for i in range(8))
    def pred(c):
        r = c.rows_out()
        assert [x[b"k"] for x in r[:4]] == [b"a0", b"a1", b"a2", b"a3"] and r[0][b"SUM(v)"] == sum(range(0, 40, 4)) + 14 and len(r) == 44
    add("grow_in_second_chunk", DICT_SQL, [first, second, TIMER], [(0, 0), (1, None)], pred=pred)
    def pred(c):
        assert [x[b"k"] for x in c.rows_out(1)] == [b"a0", b"a1"] and c.want()[2] == b"" == c.want()[5] and [x[b"k"] for x in c.rows_out(4)] == [b"a1", b"z", b"a0"]
    add("second_window", DICT_SQL, [krec("a0", 1) + krec("a1", 2), TIMER, TIMER, krec("a1", 5) + krec("z", 6) + krec("a0", 7), TIMER, TIMER], [(0, 0), (0, 0)], pred=pred)
    add("wave/one_new_group", DICT_SQL, [b"".join(krec("same", i, i) for i in range(64)), TIMER], [(0, 0)],
        pred=lambda c: need(c.rows_out() == [{b"k": b"same", b"COUNT(*)": 64, b"SUM(v)": 2016}], c.name))
    add("wave/64_new_groups", DICT_SQL, [b"".join(krec(i, i, i) for i in range(64)), TIMER], [(3, None)],
        pred=lambda c: need([x[b"k"] for x in c.rows_out()] == list(range(64)), c.name))
    # tuples that are one group unless class bytes and terminators are honoured
    pairs = [("a", "bc"), ("ab", "c"), ("ab", ""), ("abc", ""), ("", "abc")]
    ch = b"".join(krec(k, i, i, j=j) for i, (k, j) in enumerate(pairs * 2))
    add("collide/strings", DICT_SQL2, [ch, TIMER], [(0, 0)], pred=lambda c: need(len(c.rows_out()) == 5, c.name))
    ch = b"".join(krec(k, i, i) for i, k in enumerate([0.0, -0.0, 1.5, -1.5, 0.0]))
    def pred(c):
        assert [x[b"COUNT(*)"] for x in c.rows_out()] == [3, 1, 1]                   # 0.0 and -0.0 are one group
    add("collide/zero_signs", DICT_SQL, [ch, TIMER], [(0, 0)], pred=pred)
    ch = b"".join(krec(k, i, i) for i, k in enumerate([7, "7", " 7", "+7", "07", 8, "8"]))
    def pred(c):
        assert [(x[b"k"], x[b"COUNT(*)"]) for x in c.rows_out()] == [(7, 5), (8, 2)]
    add("collide/str_conv", DICT_SQL, [ch, TIMER], [(0, 0)], pred=pred)
    # a row split in two: the rows behind it (which would be new groups) are not this chunk's
    rows = [krec("g%d" % (i % 3), i, i) for i in range(20)]
    k = 11
    behind = [krec("new%d" % i, 100 + i, i) for i in range(6)]
    split = Dev(rows[:k] + [rows[k][:9], rows[k][9:]] + behind)
    nxt = krec("new3", 1, 50) + krec("g1", 2, 51) + krec("new0", 3, 52)
    def pred(c):
        assert c.steps[0].first_bad() == k and c.want()[0][0] == k
        assert [x[b"k"] for x in c.rows_out(1)] == [b"g0", b"g1", b"g2"]
        assert [x[b"k"] for x in c.rows_out(3)] == [b"new3", b"g1", b"new0"]
    add("split_row", DICT_SQL, [split, TIMER, nxt, TIMER], [(0, None), (0, None)], pred=pred, first_bad=k)
    return cs


# ------------------------------------------------------------------------------------------ values
VAL_SQL = "SELECT g, COUNT(*), SUM(v), AVG(v), MIN(v), MAX(v) FROM STREAM:s GROUP BY g;"
MINMAX_SQL = "SELECT g, MIN(v), MAX(v) FROM STREAM:s GROUP BY g;"
DBL_MAX = float.fromhex("0x1.fffffffffffffp1023")
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


def vchunk(groups):
    """[(values of group 0), ...] -> records in the order given, group by group"""
    out, i = [], 0
    for g, vals in enumerate(groups):
        for v in vals:
            out.append(rec([(P("g"), P(g)), (P("v"), v if isinstance(v, bytes) else P(v))], 1700000000 + i))
            i += 1
    return b"".join(out)


def values_cases():
    cs = []

    def add(name, groups, pred=None, sql=VAL_SQL, refused=None, **kw):
        notes = dict(kw)
        if refused is not None:
            notes["refused"] = refused
        cs.append(Case("values/" + name, sql, [vchunk(groups)], pred, notes=notes))

    tiny = float.fromhex("0x0.0000000000001p-1022")
    def sums(*want_):
        def pred(c):
            got = [x[b"SUM(v)"] for x in c.rows_out(0)]
            want = [osp._to_f32(w) if isinstance(w, float) else w for w in want_]          # a float sum leaves as binary32
            assert len(got) == len(want) and all(type(a) is type(b) and (a == b) for a, b in zip(got, want)), (c.name, got, want)
        return pred
    # the smallest subnormal: what leaves is float32, which cannot show it (0.0 in every field) -- the case runs digit 0 through the
    # kernels, it does not pin its value
    add("float/subnormal", [[tiny, tiny], [tiny, -tiny, tiny]], lambda c: need(len(c.rows_out(0)) == 2, c.name),
        f32="below float32's range: every field is 0.0, the digits are run but not seen")
    # (2^52 + 1) 2^e + (2^52 - 1) 2^e = 2^(53 + e), a float32 number: the digit shift (e + 1074) & 31 at 0, 1 and 31, each value 53
    # bits wide (two digits, three at shift 31); a wrong shift or a dropped low digit leaves another sum
    shifts = [(-178, 0), (-177, 1), (-147, 31), (-50, 0), (13, 31)]
    def pred(c):
        assert [(e + 1074) & 31 for e, _ in shifts] == [s for _, s in shifts]
        assert [x[b"SUM(v)"] for x in c.rows_out(0)] == [2.0 ** (53 + e) for e, _ in shifts]
        assert all(len(digits_touched((2 ** 52 - 1) * 2.0 ** e)) == (3 if s == 31 else 2) for e, s in shifts)
    add("float/limb_shifts", [[(2 ** 52 + 1) * 2.0 ** e, (2 ** 52 - 1) * 2.0 ** e] for e, _ in shifts], pred)
    # +-DBL_MAX cancelling down to a float32 number in an order whose every partial sum is exact: digits 63..65 and the carries
    # between them ((2^53 - 1) 2^971 - (2^53 - 2) 2^971 - 2^971 borrows through all three)
    near = float.fromhex("0x1.ffffffffffffep1023")
    add("float/dbl_max_cancel", [[DBL_MAX, -DBL_MAX, 1.5], [-DBL_MAX, DBL_MAX, -2.5], [DBL_MAX, -near, -(2.0 ** 971), 1.5], [-DBL_MAX, near, 2.0 ** 971, -0.75]],
        sums(1.5, -2.5, 1.5, -0.75))
    add("float/negative_total", [[-1.5, 0.25], [3, -8.5, 2]], sums(-1.25, -3.5))
    add("float/zero_total", [[1.5, -1.5], [-2.5, 1, 1.5]], sums(0.0, 0.0))
    add("float/carry_out_of_every_digit", [[4294967295.0, 4294967295.0], [-4294967295.0, -4294967295.0]], sums(8589934590.0, -8589934590.0),
        f32="2^33 - 2 leaves as 2^33: a lost carry is 2^32 or more away and shows")
    add("float/carry_exact", [[16777215.0 * 2 ** 9, 2.0 ** 9], [-(16777215.0 * 2 ** 18), -(2.0 ** 18)]], sums(2.0 ** 33, -(2.0 ** 42)))
    big = b"\xcf" + struct.pack(">Q", 2 ** 63 + 5)
    add("int/extremes", [[I64_MIN], [I64_MAX], [big], [I64_MIN, I64_MAX]], sums(I64_MIN, I64_MAX, I64_MIN + 5, -1))
    add("int/sum_wraps", [[I64_MAX, 1], [I64_MIN, -1], [I64_MAX, I64_MAX, 2]], sums(I64_MIN, I64_MAX, 0))
    add("int/then_float", [[5, 7, 0.5], [-3, 2 ** 20, 0.25]], sums(12.5, float(2 ** 20 - 3) + 0.25))
    add("int/float_first", [[0.5, 5, 7], [0.0, 5, 7]], sums(12.5, 12))
    # the reference's sum is a wrapping int64 until the first non-zero float arrives, a double from there on: the same values
    # give other answers in other orders, and the device has to give this order's
    add("wrap/before_float", [[2 ** 62, 2 ** 62, 2.0 ** 40], [I64_MAX, 1, -(2.0 ** 40)]], sums(-(2.0 ** 63) + 2.0 ** 40, -(2.0 ** 63) - 2.0 ** 40))
    add("wrap/float_first", [[2.0 ** 40, 2 ** 62, 2 ** 62]], sums(2.0 ** 63 + 2.0 ** 40))
    add("wrap/and_back", [[2 ** 62, 2 ** 62, -2 ** 62, 2.0 ** 40], [2 ** 62, 2 ** 62, 2.0 ** 40, 2 ** 62, 2 ** 62]], sums(2.0 ** 62 + 2.0 ** 40, 2.0 ** 40))
    add("wrap/negative", [[-2 ** 62, -2 ** 62, -2 ** 62, 2.0 ** 40], [I64_MIN, -1, 1, I64_MIN, 2.0 ** 40]], sums(2.0 ** 62 + 2.0 ** 40, 2.0 ** 40))
    add("wrap/twice", [[I64_MAX, I64_MAX, I64_MAX, I64_MAX, 4, 3, 2.0 ** 20, 5]], sums(2.0 ** 20 + 8))
    # integers on both sides of the float, below and above 2^32: only those ahead of it wrap
    add("wrap/ints_behind_the_float", [[2 ** 62, 2 ** 62, 2 ** 40, 2.0 ** 41, 2 ** 42, -2 ** 62], [2 ** 62, 2 ** 62, 2 ** 62, 2 ** 62, 5, 0.5, 7, -4]],
        sums(-(2.0 ** 63) - 2.0 ** 62 + 7 * 2.0 ** 40, 8.5))
    inf = float("inf")
    add("minmax/mixed", [[3, -0.0, 2.5], [2 ** 53 + 1, 2.0 ** 53], [-inf, 5, inf], [-(2 ** 53) - 1, -(2.0 ** 53), 0.5], [I64_MIN, -1e300], [I64_MAX, 1e300]], sql=MINMAX_SQL,
        pred=lambda c: need([(x[b"MIN(v)"], x[b"MAX(v)"]) for x in c.rows_out(0)][:3] == [(0.0, 3.0), (2.0 ** 53, 2.0 ** 53), (-inf, inf)], c.name))
    strs = ["9223372036854775807", "9223372036854775808", "-9223372036854775808", "-922337203685477580", "+5", "-", " ", "\x005", "5\x006", "1.", ".5", " 12", "1.5.1"]
    def pred(c):
        r = {x[b"g"]: x[b"SUM(v)"] for x in c.rows_out(0)}
        assert [len(s) for s in strs[:4]] == [19, 19, 20, 19]
        assert (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12]) == (I64_MIN, 1, 1, -922337203685477579, 6, 1, 1, 1, 6, 2.0, 1.5, 13, 1), r
    add("strings/boundaries", [[s, 1] for s in strs], pred, deferred=True)
    T = 2 ** 31
    times = [(T - 1, 0), (T, 0), (T, 500000000), (2 ** 32 - 3, 999999999), (5, 0)]      # (0xfffffffe / 0xffffffff seconds are group markers)
    ch = b"".join(rec(body({"v": i}), s, ns) for i, (s, ns) in enumerate(times))
    for op, n in ((">", 2), ("<=", 3), ("=", 1)):
        cs.append(Case("values/time/%s" % {">": "gt", "<=": "lte", "=": "eq"}[op], "SELECT COUNT(*), SUM(v) FROM STREAM:s WHERE @record.time() %s 2147483648.5;" % op, [ch],
                       lambda c, n=n: need(c.want()[0][0] == n, c.name)))
    return cs


# ------------------------------------------------------------------------------------------ grid
GRID_SQL = "SELECT g, COUNT(*), SUM(v), MIN(v), MAX(v) FROM STREAM:s WINDOW TUMBLING (5 SECOND) GROUP BY g;"
GRID_BLOCK = 512
GRID_NAMES = ("grid/second_trip", "grid/spill", "grid/one_slot", "grid/normalize_second_trip")
SIX = ", ".join("SUM(f%d)" % i for i in range(6))
SPILL_SQL = "SELECT g, COUNT(*), %s FROM STREAM:s WINDOW TUMBLING (5 SECOND) GROUP BY g;" % SIX


def grid_rows(cus):
    return max(2 * cus * SP_BLOCK, GENERIC_GRID[0] * GENERIC_GRID[1]) + 65


def grid_block():
    return [rec(body({"g": i % 7, "v": i}), 1700000000) for i in range(GRID_BLOCK)]


def grid_tail():
    """65 rows of new groups, two of them with a decimal string (k_sp_generic redoes those)"""
    return [rec(body({"g": 100 + i % 9, "v": "%d.5" % i if i in (3, 64) else i}), 1700000001) for i in range(65)]


def scaled_answer(repeat):
    """the oracle's answer for `repeat` copies of the integer-only block and the tail behind them, from its answers for ONE block and
    for the tail alone: COUNT and SUM of the block's groups times `repeat` (MIN / MAX and the order stay), then the tail's groups"""
    t = osp.Task(GRID_SQL)
    n_block = t.do(b"".join(grid_block()))[0]
    u = msgpack.Unpacker(raw=True, strict_map_key=False)
    u.feed(t.timer())
    out = b""
    for head, m in u:
        out += b"\x92\xd7\x00" + head.data + bytes([0x80 | len(m)])
        for k, v in m.items():
            out += osp._pack_str(k) + osp._pack_int(v * repeat if k in (b"COUNT(*)", b"SUM(v)") else v)
    t = osp.Task(GRID_SQL)
    n_tail = t.do(b"".join(grid_tail()))[0]
    return [(n_block * repeat + n_tail, b""), out + t.timer()]


class ScaledCase(Case):
    """`repeat` blocks + the tail; want() is scaled_answer(repeat) (tests/test_sp_chunks.py proves the scaling at small counts)"""

    def __init__(self, name, repeat, pred, notes):
        rows = grid_block() * repeat + grid_tail()
        Case.__init__(self, name, GRID_SQL, [Dev(rows), TIMER], pred, notes=notes, ref=False)
        self.repeat = repeat

    def want(self):
        if self._want is None:
            self._want, self.inexact, self.f32_rounds = scaled_answer(self.repeat), None, []
        return self._want


def digits_touched(v):
    """the base-2^32 digits of |v| / 2^-1074 that are not zero: the words sp_add_digits adds to"""
    n = Fraction(abs(v)) * 2 ** 1074
    assert n.denominator == 1
    n, j, out = int(n), 0, []
    while n:
        if n & 0xFFFFFFFF:
            out.append(j)
        n >>= 32
        j += 1
    return out


def combiner_words(rows_values):
    """distinct row words k_sp_aggregate's combiner is asked for by rows of (group, [six float values]): the group's record count,
    and per source the float count and the touched digits"""
    words = set()
    for g, vals in rows_values:
        words.add((g, "records"))
        for s, v in enumerate(vals):
            words.add((g, s, "nflt"))
            words.update((g, s, j) for j in digits_touched(v))
    return words


def grid_cases(cus=NOMINAL_CUS):
    cs = []
    n = grid_rows(cus)
    repeat = (n - 65) // GRID_BLOCK
    def pred(c, n=n, cus=cus):
        d = c.steps[0]
        assert len(d.rows) == n == repeat * GRID_BLOCK + 65
        assert n > 2 * cus * SP_BLOCK and n > 2 * cus * LIM["L2M_AGG_BLOCK"] and n - 65 >= GENERIC_GRID[0] * GENERIC_GRID[1]      # a second trip in all three
        assert sum(1 for r in d.rows[-65:] if b".5" in r) == 2 and len(c.rows_out()) == 7 + 9
    cs.append(ScaledCase("grid/second_trip", repeat, pred, {"deferred": True, "cus": cus}))
    # one workgroup's first L2M_AGG_BLOCK rows: 256 groups x 6 float sources
    def frow(g, i):
        # bits on both sides of 2^14, where digit 34 begins: two digits a value, and twice the value is a float32 number
        vals = [float(2 ** 14 * (i + 1) + 2 ** 4 * (3 * i + s + 1)) if g == i else s + 0.5 for s in range(6)]          # one group: sums of 512 stay exact
        return (g, vals), rec(body(dict({"g": g}, **{"f%d" % s: vals[s] for s in range(6)})), 1700000000)
    for name, gof in (("spill", lambda i: i), ("one_slot", lambda i: 0)):
        rows = [frow(gof(i % 256), i % 256) for i in range(512)]                     # every value twice: 2 v is exact
        def pred(c, rows=rows, name=name):
            w = combiner_words([r[0] for r in rows[:LIM["L2M_AGG_BLOCK"]]])
            if name == "spill":
                assert len(w) > LIM["L2M_AGG_SLOTS"], len(w)
            else:
                assert len(w) < 64 and len({r[0][0] for r in rows}) == 1
        cs.append(Case("grid/" + name, SPILL_SQL, [Dev([r[1] for r in rows]), TIMER], pred))
    ng = NORMALIZE_GRID[0] * NORMALIZE_GRID[1] // 6 + 70
    rows = [rec(body(dict({"g": i % ng}, **{"f%d" % s: 4294967295.0 for s in range(6)})), 1700000000) for i in range(2 * ng)]
    def pred(c, ng=ng):
        assert ng * 6 > NORMALIZE_GRID[0] * NORMALIZE_GRID[1] and len(c.rows_out()) == ng
        assert all(x[b"SUM(f5)"] == osp._to_f32(8589934590.0) for x in c.rows_out())               # two (2^32 - 1): a carry out of both touched digits
    cs.append(Case("grid/normalize_second_trip", SPILL_SQL, [Dev(rows), TIMER], pred, notes={"f32": "2^33 - 2 leaves as 2^33: a lost carry is 2^32 or more away"}))
    assert tuple(c.name for c in cs) == GRID_NAMES
    return cs


# ------------------------------------------------------------------------------------------ all of them
_BUILD = {"staging": lambda: staging_cases(False) + staging_cases(True), "keys": keys_cases, "multiplicity": multiplicity_cases,
          "dictionary": dictionary_cases, "values": values_cases, "grid": grid_cases}
_CACHE = {}


def cases(group):
    if group not in _CACHE:
        _CACHE[group] = _BUILD[group]()
    return _CACHE[group]


def all_cases():
    return [c for g in GROUPS for c in cases(g)]
