"""Named cases for filter_log_to_metrics' extract, stale, aggregate and dictionary kernels (csrc/l2m_kernels.inc, csrc/l2m_dev.inc): every
case sits on one edge of that code, and carries a predicate that says so from the case alone --

  columns   (sid, val) columns for flbgpu_l2m_stale_dev / flbgpu_l2m_aggregate_dev, with the plain models they are compared against:
            stale_model (a sequential walk), AggModel (first index, last index + 1 and value, count, NaN / +Inf / -Inf counts, buckets
            by cmetrics' walk down from the top bound, the sum as ONE Python integer in units of 2^-1074) and round_fraction
            (fractions.Fraction -> binary64, nearest-even, overflow to +-inf)
  records   chunks for FilterLogToMetrics against oracle_binding.L2M: k_l2m_extract's staging (the fit test per align, records over the
            tile, the chunk's end at every residue mod 16, row counts, the second grid-stride trip), k_l2m_generic's second trip, the
            dictionary insert

tests/test_l2m_chunks.py runs the predicates and holds the models against the oracle on the CPU; tests/test_l2m_edges_gpu.py runs the
cases on the device.  The constants below restate the sources'; test_l2m_chunks.py reads them out of dev.hpp / l2m_kernels.inc and
compares, so a changed constant fails there and does not silently move a case off its edge."""
import math
import struct
from fractions import Fraction

import numpy as np

from synth import mp, v2_record, Raw

# ------------------------------------------------------------------------------------------ the sources' constants
L2M_BLOCK = 256                  # k_l2m_extract: rows per workgroup and trip
L2M_TILE = 18432                 # LDS bytes per wave
L2M_GENERIC_GRID = 4096          # launch_l2m_generic: at most 4096 workgroups of 64 lanes
L2M_ST_BLOCK, L2M_ST_ITEMS = 256, 8
L2M_ST_TILE = L2M_ST_BLOCK * L2M_ST_ITEMS
L2M_SPINE = 1024                 # k_l2m_stale_spine: tiles per trip
L2M_AGG_BLOCK = 256
L2M_AGG_SLOTS = 4096
L2M_AGG_PROBES = 4
L2M_NLIMB = 68
L2M_W_FIRST, L2M_W_LASTIDX, L2M_W_LASTVAL, L2M_W_COUNT, L2M_W_SPECIAL, L2M_W_LIMB = 0, 1, 2, 3, 4, 7
L2M_W_BUCKET = L2M_W_LIMB + L2M_NLIMB
NONE, DEFER, STALE = 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000
COUNTER, GAUGE, HISTOGRAM = 0, 1, 2
MODE_NAMES = {COUNTER: "counter", GAUGE: "gauge", HISTOGRAM: "histogram"}
NOBAD = 2 ** 64 - 1
M64 = 2 ** 64 - 1
DEFAULT_BOUNDS = [0.005, 0.01, 0.025, 0.05, 0.1, 0.25, 0.5, 1.0, 2.5, 5.0, 10.0]
DBL_MAX = 1.7976931348623157e308


def row_words(mode, nb=0):
    return L2M_W_BUCKET + nb + 1 if mode == HISTOGRAM else L2M_W_SPECIAL


def f2b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def b2f(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


# ------------------------------------------------------------------------------------------ the plain models
def stale_model(sid, val, first_bad=NOBAD):
    """row i flagged STALE takes the value of the closest earlier row that assigned one (else 0.0) and loses the flag; nothing at or
    behind first_bad; NONE / DEFER rows neither assign nor take.  A sequential walk over the rows that are not NONE."""
    sid, val = np.array(sid, dtype=np.uint32), np.array(val, dtype=np.uint64)
    lim = min(first_bad, len(sid))
    last = None
    for i in np.nonzero(sid[:lim] != NONE)[0]:
        s = int(sid[i])
        if s < STALE:
            last = i
        elif s != DEFER:
            val[i] = val[last] if last is not None else 0
            sid[i] = s & ~STALE
    return sid, val


def round_fraction(x):
    """the binary64 nearest to the rational x (ties to even, overflow to +-inf), as a float"""
    x = Fraction(x)
    if x == 0:
        return 0.0
    neg, x = x < 0, abs(x)
    # e: the weight of the result's last mantissa bit -- 2^52 <= x / 2^e < 2^53, but never under the subnormals' 2^-1074
    e = (x.numerator.bit_length() - x.denominator.bit_length()) - 53
    while x >= Fraction(2) ** (e + 53): e += 1
    while x < Fraction(2) ** (e + 52): e -= 1
    e = max(e, -1074)
    y = x / Fraction(2) ** e
    q, r = divmod(y.numerator, y.denominator)
    twice = 2 * r
    if twice > y.denominator or (twice == y.denominator and (q & 1)):
        q += 1
    if q == 2 ** 53:
        q, e = 2 ** 52, e + 1
    if e + 53 > 1024:
        res = math.inf
    else:
        res = math.ldexp(q, e)
        assert Fraction(res) == Fraction(q) * Fraction(2) ** e
    return -res if neg else res


def to_units(v):
    """the finite double v as an integer number of 2^-1074 (every double is one)"""
    m, e = math.frexp(v)
    M, sh = int(math.ldexp(m, 53)), e - 53 + 1074
    if sh >= 0:
        return M << sh
    assert (M >> -sh) << -sh == M
    return M >> -sh


def bucket_of(v, bounds):
    """cmt_histogram_observe: walking down from the top bound, every bucket is incremented until v > bound -- the lowest bucket that
    is incremented (the rows keep the buckets non-cumulative)"""
    b = len(bounds)
    for k in range(len(bounds) - 1, -1, -1):
        if v > bounds[k]:
            break
        b = k
    return b


class AggModel:
    """the series rows of one filter, word for word as the device keeps them between calls"""

    def __init__(self, mode, nseries, bounds=()):
        self.mode, self.ns, self.bounds = mode, nseries, list(bounds) if mode == HISTOGRAM else []
        self.nb = len(self.bounds)
        self.first = [None] * nseries          # smallest global index
        self.last = [0] * nseries              # largest global index + 1 (gauge)
        self.lastval = [0] * nseries
        self.count = [0] * nseries             # (counter)
        self.special = [[0, 0, 0] for _ in range(nseries)]
        self.sum = [0] * nseries               # units of 2^-1074
        self.buckets = [[0] * (self.nb + 1) for _ in range(nseries)]

    def call(self, sid, val=None, first_bad=NOBAD, idx_base=0):
        n = len(sid)
        lim = min(first_bad, n)
        for i in np.nonzero(np.asarray(sid[:lim], dtype=np.uint32) < STALE)[0]:
            i = int(i)
            s = int(sid[i])
            g = (idx_base + i) & M64
            if self.first[s] is None or g < self.first[s]:
                self.first[s] = g
            if self.mode == COUNTER:
                self.count[s] += 1
            elif self.mode == GAUGE:
                self.last[s] = max(self.last[s], g + 1)
            else:
                bits = int(val[i])
                v = b2f(bits)
                self.buckets[s][bucket_of(v, self.bounds)] += 1
                if v != v: self.special[s][0] += 1
                elif v == math.inf: self.special[s][1] += 1
                elif v == -math.inf: self.special[s][2] += 1
                else:
                    self.sum[s] += to_units(v)
        if self.mode == GAUGE:                 # the row that holds the largest index hands over its value, if it is of this call
            for s in range(self.ns):
                li = self.last[s]
                if li > idx_base and li - 1 - idx_base < n:
                    self.lastval[s] = int(val[li - 1 - idx_base])

    def rows(self):
        W = row_words(self.mode, self.nb)
        out = np.zeros((self.ns, W), dtype=np.uint64)
        for s in range(self.ns):
            out[s, L2M_W_FIRST] = 0 if self.first[s] is None else (~self.first[s]) & M64
            out[s, L2M_W_LASTIDX] = self.last[s]
            out[s, L2M_W_LASTVAL] = self.lastval[s]
            out[s, L2M_W_COUNT] = self.count[s]
            if self.mode == HISTOGRAM:
                for w in range(3): out[s, L2M_W_SPECIAL + w] = self.special[s][w]
                t = self.sum[s]
                for j in range(L2M_NLIMB - 1): out[s, L2M_W_LIMB + j] = (t >> (32 * j)) & 0xFFFFFFFF
                out[s, L2M_W_LIMB + L2M_NLIMB - 1] = (t >> (32 * (L2M_NLIMB - 1))) & M64       # the top digit keeps the sign
                for b in range(self.nb + 1): out[s, L2M_W_BUCKET + b] = self.buckets[s][b]
        return out

    def final(self, s):
        """what cmetrics would hold for series s: dict(value=, buckets=[cumulative..], count=, sum=)"""
        if self.mode == COUNTER:
            return dict(value=float(min(self.count[s], 2 ** 53)))
        if self.mode == GAUGE:
            return dict(value=b2f(self.lastval[s]))
        cum, run = [], 0
        for c in self.buckets[s]:
            run += c; cum.append(run)
        nan, pinf, ninf = self.special[s]
        if nan or (pinf and ninf): sm = math.nan
        elif pinf: sm = math.inf
        elif ninf: sm = -math.inf
        else: sm = round_fraction(Fraction(self.sum[s]) / Fraction(2) ** 1074)
        return dict(buckets=cum, count=run, sum=sm)

    def order(self):
        """the series that exist, in first-appearance order"""
        return sorted((s for s in range(self.ns) if self.first[s] is not None), key=lambda s: self.first[s])


# ------------------------------------------------------------------------------------------ column cases
class Case:
    def __init__(self, name, pred=None, **kw):
        self.name, self.pred = name, pred
        self.__dict__.update(kw)

    def check(self):
        if self.pred is not None:
            assert self.pred(self), self.name
        return self

    def __repr__(self):
        return self.name


def _tiles(n):
    return (n + L2M_ST_TILE - 1) // L2M_ST_TILE


def _stale_case(name, n, put, first_bad=NOBAD, pred=None, fill=0):
    """`put`: {row: sid}; the other rows are NONE.  Every row's value is its own index + 1 as a double (a stale row's too: it must be
    overwritten), so a value names the row it came from."""
    sid = np.full(n, NONE, dtype=np.uint32)
    if fill:                                                # a sprinkling of assigning / stale / deferred rows, one in `fill`
        rs = np.random.RandomState(n % 65521)
        pick = rs.choice(n, n // fill, replace=False)
        kind = rs.randint(0, 8, len(pick))
        sid[pick] = np.where(kind < 3, 5, np.where(kind < 7, 5 | STALE, DEFER)).astype(np.uint32)
    for r, s in put.items():
        sid[r] = s
    val = (np.arange(n, dtype=np.float64) + 1.0).view(np.uint64)
    return Case("stale/" + name, pred, sid=sid, val=val, first_bad=first_bad, n=n)


def _src_of(c, row):
    """the row a stale row must take its value from, by a backwards walk (None: 0.0)"""
    idx = np.nonzero(c.sid[:min(row, c.first_bad, c.n)] < STALE)[0]
    return int(idx[-1]) if len(idx) else None


def stale_cases():
    T, S = L2M_ST_TILE, L2M_SPINE
    cs = []
    for n in (1, T - 1, T, T + 1):
        cs.append(_stale_case("n=%d/stale_only" % n, n, {n - 1: 3 | STALE}, pred=lambda c: _src_of(c, c.n - 1) is None and _tiles(c.n) == (c.n + T - 1) // T))
        if n > 1:
            cs.append(_stale_case("n=%d/first_assigns_last_takes" % n, n, {0: 1, n - 1: 3 | STALE}, pred=lambda c: _src_of(c, c.n - 1) == 0))
    for n in (S * T - T, S * T, S * T + T):
        # the last tile's first row takes from the first tile's first row: past 1024 tiles only the spine's carry brings it there
        cs.append(_stale_case("n=%d/tiles=%d" % (n, _tiles(n)), n, {0: 1, n - T: 2 | STALE, n - 1: 7 | STALE, n - 2: 9}, fill=97,
                              pred=lambda c, n=n: _tiles(c.n) == n // T and c.sid[c.n - T] & STALE and c.sid[c.n - 1] & STALE))
    n = (S + 9) * T + 5
    cs.append(_stale_case("spine/source_1030_tiles_back", n, {T + 1: 4, (S + 7) * T: 1 | STALE, (S + 7) * T + 1: 2, (S + 8) * T + 9: 1 | STALE, n - 1: 6 | STALE},
                          pred=lambda c: _tiles(c.n) == S + 10 and _src_of(c, (S + 7) * T) == T + 1 and ((S + 7) * T) // T - (T + 1) // T == S + 6 == 1030
                          and _src_of(c, (S + 8) * T + 9) == (S + 7) * T + 1 and _src_of(c, c.n - 1) == (S + 7) * T + 1))
    cs.append(_stale_case("spine/tile_count_1025", S * T + 1, {S * T - 1: 4, S * T: 1 | STALE},
                          pred=lambda c: _tiles(c.n) == S + 1 and _src_of(c, S * T) == S * T - 1))
    cs.append(_stale_case("spine/no_source_in_second_trip", S * T + 2 * T, {S * T + T + 3: 1 | STALE, 5: DEFER, 6: 1 | STALE},
                          pred=lambda c: _src_of(c, S * T + T + 3) is None))
    cs.append(_stale_case("tile/source_in_previous_tiles_last_slot", 3 * T, {T - 1: 4, T: 1 | STALE, 2 * T - 1: 2 | STALE, 2 * T: 3 | STALE},
                          pred=lambda c: _src_of(c, T) == T - 1 and _src_of(c, 2 * T) == T - 1))
    cs.append(_stale_case("tile/source_3_tiles_back", 5 * T, {T + 7: 4, 4 * T + 1: 1 | STALE, 4 * T + 2: 0, 4 * T + 3: 9 | STALE},
                          pred=lambda c: _src_of(c, 4 * T + 1) == T + 7 and _src_of(c, 4 * T + 3) == 4 * T + 2))
    cs.append(_stale_case("tile/none_and_defer_between", T + 20, {T - 3: 8, T - 2: DEFER, T - 1: NONE, T: DEFER, T + 1: 0 | STALE, T + 2: DEFER, T + 3: 3 | STALE},
                          pred=lambda c: _src_of(c, T + 1) == T - 3 and _src_of(c, T + 3) == T - 3))
    cs.append(_stale_case("tile/thread_edges", T, {7: 1, 8: 1 | STALE, 15: 2 | STALE, 16: 3, 63 * 8 + 7: 4, 64 * 8: 5 | STALE, 255 * 8: 6 | STALE, 255 * 8 + 7: 7 | STALE},
                          pred=lambda c: _src_of(c, 8) == 7 and _src_of(c, 64 * 8) == 63 * 8 + 7 and _src_of(c, 255 * 8 + 7) == 63 * 8 + 7))
    cs.append(_stale_case("tile/assigning_rows_keep_their_values", 2 * T, {i: (i % 5) for i in range(0, 2 * T, 3)}, fill=4,
                          pred=lambda c: True))
    base = {0: 1, 5: 1 | STALE, T - 1: 2, T: 1 | STALE, T + 9: 3, T + 10: 2 | STALE, 2 * T + 4: 5 | STALE}
    for fb, what in ((0, "at_0"), (T + 10, "inside_a_tile"), (T + 11, "behind_a_taker"), (T, "at_a_tile_edge"), (2 * T + 5, "at_n"), (6, "inside_first_tile")):
        cs.append(_stale_case("first_bad/" + what, 2 * T + 5, base, first_bad=fb, pred=lambda c, fb=fb: c.first_bad == fb <= c.n))
    cs.append(_stale_case("first_bad/source_behind_it", 3 * T, {T + 1: 9, 2 * T: 1 | STALE, 5: 3, 7: 4 | STALE}, first_bad=T,
                          pred=lambda c: c.sid[2 * T] & STALE and c.first_bad < 2 * T))
    return cs


def combiner_hash(word):
    """L2mCombiner::upd: the first LDS slot of row word `word`"""
    return (((word + 1) * 2654435761) & 0xFFFFFFFF) >> 20


def colliding_series(mode, nb=0, want=6):
    """`want` series whose combined word (the counter's count, the gauge's last index) starts its probes at ONE slot: four of them fill
    the four probed slots, the others must take the global path whatever the order the workgroup's lanes arrive in"""
    W, word = row_words(mode, nb), (L2M_W_COUNT if mode == COUNTER else L2M_W_LASTIDX)
    seen = {}
    for s in range(1 << 20):
        h = combiner_hash(s * W + word)
        seen.setdefault(h, []).append(s)
        if len(seen[h]) == want:
            return seen[h]
    raise AssertionError("no collision found")


def pow2(j, sh):
    """the double whose single set bit is bit sh of sum digit j (E + 1074 == 32 j + sh)"""
    return math.ldexp(1.0, 32 * j + sh - 1074)


def _agg(name, mode, nseries, calls, bounds=(), pred=None, records=None, exact=True):
    """calls: [(sid, val or None, first_bad, idx_base)]"""
    cc = []
    for sid, val, fb, base in calls:
        sid = np.asarray(sid, dtype=np.uint32)
        if val is None:
            val = np.arange(len(sid), dtype=np.float64) + 1.0
        val = np.asarray(val)
        val = val.view(np.uint64) if val.dtype == np.float64 else val.astype(np.uint64)
        cc.append((sid, val, fb, base))
    n = max(len(c[0]) for c in cc)
    return Case("agg/%s/%s" % (MODE_NAMES[mode], name), pred, mode=mode, nseries=nseries, calls=cc, bounds=list(bounds) if mode == HISTOGRAM else [],
                records=(n <= 1024 and all(c[3] == sum(len(x[0]) for x in cc[:k]) for k, c in enumerate(cc))) if records is None else records, exact=exact)


def _model_of(c):
    m = AggModel(c.mode, c.nseries, c.bounds)
    for sid, val, fb, base in c.calls:
        m.call(sid, val, fb, base)
    return m


HIST_VALUES = [DBL_MAX, -DBL_MAX, 5e-324, -5e-324, 0.0, -0.0, math.nan, math.inf, -math.inf,
               # a 53-bit mantissa at sh = 31: E + 1074 = 32 j + 31 with E the weight of the mantissa's LAST bit
               math.ldexp(float(2 ** 53 - 1), 32 * 20 + 31 - 1074), -math.ldexp(float(2 ** 52 + 1), 32 * 40 + 31 - 1074)] + \
              [sg * math.ldexp(1.0, 32 * j + sh - 1074 + 52) for j in (0, 31, 62) for sh in (0, 1, 31) for sg in (1, -1)] + \
              [sg * pow2(j, sh) for j in (0, 33, 63) for sh in (0, 1, 31) for sg in (1, -1)]


def wg_of(i, n, cus):
    """the k_l2m_aggregate workgroup that visits row i of n"""
    grid = max(1, min(2 * cus, (n + L2M_AGG_BLOCK - 1) // L2M_AGG_BLOCK))
    return (i // L2M_AGG_BLOCK) % grid


def agg_cases(cus=256):
    """the aggregate cases; `cus` (the device's compute units) places the grid-stride edge: 2 x CUs x 256 rows"""
    B = L2M_AGG_BLOCK
    G = 2 * cus * B
    cs = []
    for mode in (COUNTER, GAUGE, HISTOGRAM):
        bd = DEFAULT_BOUNDS
        for n in (1, B - 1, B, B + 1, G - 1, G, G + 1):
            ns = 7
            sid = (np.arange(n, dtype=np.uint64) * 2654435761 % 11).astype(np.uint32)
            sid = np.where(sid >= ns, np.where(sid == 7, NONE, np.where(sid == 8, DEFER, (sid - 9) | STALE)), sid).astype(np.uint32)
            val = ((np.arange(n) % 23) - 11) * 0.125                                  # dyadic: every order of adding them is exact
            cs.append(_agg("n=%d" % n, mode, ns, [(sid, val, NOBAD, 0)], bd, pred=lambda c, n=n: len(c.calls[0][0]) == n))
        n = 3 * B + 1
        cs.append(_agg("one_series_takes_every_row", mode, 3, [(np.full(n, 1), ((np.arange(n) % 9) - 4) * 0.5, NOBAD, 0)], bd,
                       pred=lambda c: set(c.calls[0][0]) == {1}))
        cs.append(_agg("as_many_series_as_rows", mode, n, [(np.random.RandomState(1).permutation(n), ((np.arange(n) % 9) - 4) * 0.5, NOBAD, 0)], bd,
                       pred=lambda c: len(set(c.calls[0][0])) == len(c.calls[0][0])))
        cs.append(_agg("first_bad_cuts_the_call", mode, 4, [(np.arange(n) % 4, None, B + 3, 0), (np.arange(n) % 3, None, 0, n), (np.arange(7) % 4, None, 7, 2 * n)], bd,
                       pred=lambda c: c.calls[0][2] < len(c.calls[0][0]) and c.calls[1][2] == 0))
        for base in (0, 2 ** 32 - 1 - 5, 2 ** 63 - 3, 2 ** 63 + 12345):
            # two chained calls: series 0 and 1 in both, 2 only in the first (untouched by the second), 3 only in the second
            s1, s2 = np.array([0, 1, 2, 2, 1, 0], dtype=np.uint32), np.array([1, 3, 0, NONE, 3], dtype=np.uint32)
            cs.append(_agg("idx_base=%d" % base, mode, 5, [(s1, None, NOBAD, base), (s2, None, NOBAD, base + 6)], bd,
                           pred=lambda c, base=base: c.calls[1][3] == base + 6 and (base != 2 ** 32 - 6 or c.calls[1][3] == 2 ** 32)))
    # ---- the combiner: forced collisions for both flavours, in one workgroup and over two
    for mode in (COUNTER, GAUGE):
        six = colliding_series(mode)
        for n in (240, 2 * B):
            sid = np.array([six[i % 6] for i in range(n)], dtype=np.uint32)
            cs.append(_agg("six_series_on_one_slot/n=%d" % n, mode, max(six) + 1, [(sid, None, NOBAD, 0)], records=False,
                           pred=lambda c, mode=mode: len({combiner_hash(int(s) * 4 + (L2M_W_COUNT if mode == COUNTER else L2M_W_LASTIDX)) for s in set(c.calls[0][0][:B])}) == 1
                           and len(set(c.calls[0][0][:B])) == 6 > L2M_AGG_PROBES))
    # more distinct words in ONE workgroup than the combiner has slots (ADD flavour): workgroup 0's rows are distinct series with a
    # bucket and three sum digits each, every other row is no observation; the rest of the table must go the global way
    trips = 5
    n = G * trips
    sid = np.full(n, NONE, dtype=np.uint32)
    mine = np.nonzero((np.arange(n) // B) % (2 * cus) == 0)[0]
    sid[mine] = np.arange(len(mine), dtype=np.uint32)
    val = np.zeros(n)
    val[mine] = [math.ldexp(float(2 ** 52 + 2 ** 30 + 1 + 2 * k), 20 - 52) * (-1 if k % 3 == 0 else 1) for k in range(len(mine))]

    def full_table(c, cus=cus):
        sid, val = c.calls[0][0], c.calls[0][1]
        W, words = row_words(HISTOGRAM, 1), set()
        for i in np.nonzero(sid < STALE)[0]:
            if wg_of(int(i), len(sid), cus) != 0: return False
            m = AggModel(HISTOGRAM, 1, [1.0]); m.call([0], [val[i]])
            r = m.rows()[0]
            mag = abs(m.sum[0])
            words |= {int(sid[i]) * W + L2M_W_LIMB + j for j in range(L2M_NLIMB) if (mag >> (32 * j)) & 0xFFFFFFFF}
            words.add(int(sid[i]) * W + L2M_W_BUCKET + int(np.nonzero(r[L2M_W_BUCKET:])[0][0]))
        return len(words) > L2M_AGG_SLOTS
    cs.append(_agg("more_words_than_slots_in_one_workgroup", HISTOGRAM, len(mine), [(sid, val, NOBAD, 0)], [1.0], pred=full_table, records=False))
    # ---- sums that cancel: inside one workgroup (the LDS value is 0 at the flush) and across two (two flushes that cancel in the row)
    v = [3.5, math.ldexp(1.0, 700), DBL_MAX, 5e-324]
    sid = np.full(2 * B, 1, dtype=np.uint32); val = np.zeros(2 * B)
    sid[8:] = NONE
    val[:8] = [v[0], -v[0], v[1], -v[1], v[2], -v[2], v[3], -v[3]]
    cs.append(_agg("cancels_inside_one_workgroup", HISTOGRAM, 2, [(sid, val, NOBAD, 0)], bd,
                   pred=lambda c: _model_of(c).sum[1] == 0 and max(np.nonzero(c.calls[0][0] < STALE)[0]) < B))
    sid = np.full(2 * B, NONE, dtype=np.uint32); val = np.zeros(2 * B)
    sid[:4] = 1; sid[B:B + 4] = 1
    val[:4] = v; val[B:B + 4] = [-x for x in v]
    cs.append(_agg("cancels_across_two_workgroups", HISTOGRAM, 2, [(sid, val, NOBAD, 0)], bd, exact=False,       # (in this order the sequential sum is not exact)
                   pred=lambda c: _model_of(c).sum[1] == 0 and {int(i) // B for i in np.nonzero(c.calls[0][0] < STALE)[0]} == {0, 1}))
    # ---- gauge: who hands over the value
    n = 4 * B
    sid = np.full(n, NONE, dtype=np.uint32); sid[0] = 0; sid[5] = 1; sid[n - 1] = 0; sid[n - 2] = 2
    cs.append(_agg("last_writer_in_the_last_workgroup", GAUGE, 4, [(sid, None, NOBAD, 0)],
                   pred=lambda c: c.calls[0][0][-1] == 0 and c.calls[0][0][0] == 0))
    s1 = np.array([0, 1, 2, 1], dtype=np.uint32)
    cs.append(_agg("last_writer_in_an_earlier_call", GAUGE, 4, [(s1, [1.5, 2.5, 3.5, 4.5], NOBAD, 100), (np.array([0, NONE, 2 | STALE, DEFER, 0], dtype=np.uint32), [9.0, 8.0, 7.0, 6.0, 5.0], NOBAD, 104),
                                                                 (np.array([3], dtype=np.uint32), [77.0], NOBAD, 109)], records=False,
                   # series 1 was written last by the LAST row of call 1: its index + 1 is call 2's idx_base; series 2's later row is stale-flagged
                   pred=lambda c: _model_of(c).last[1] == 104 and _model_of(c).lastval[1] == f2b(4.5) and _model_of(c).lastval[2] == f2b(3.5)))
    cs.append(_agg("last_candidate_behind_first_bad", GAUGE, 3, [(np.array([0, 1, 0, 1, 0], dtype=np.uint32), [1.0, 2.0, 3.0, 4.0, 5.0], 3, 0),
                                                               (np.array([1, 1], dtype=np.uint32), [6.0, 7.0], 1, 5)], records=False,
                   pred=lambda c: [b2f(x) for x in _model_of(c).lastval] == [3.0, 6.0, 0.0]))
    # ---- histogram values: the digit edges, one series per value and all of them in one series
    for nb, bd in ((1, [0.0]), (11, DEFAULT_BOUNDS), (64, [math.ldexp(1.0, k) for k in range(-32, 32)])):
        edge = []
        for b in bd[:3] + bd[-2:]:
            edge += [b, math.nextafter(b, math.inf), math.nextafter(b, -math.inf), -b]
        vals = edge + [0.0, -0.0, math.nan, math.inf, -math.inf, DBL_MAX, -DBL_MAX, 5e-324, -5e-324]
        cs.append(_agg("bucket_edges/nb=%d" % nb, HISTOGRAM, len(vals) + 1, [(np.arange(len(vals)), vals, NOBAD, 0), (np.full(len(vals), len(vals)), vals, NOBAD, len(vals))], bd,
                       pred=lambda c, bd=bd: len(c.bounds) == len(bd) and any(b2f(x) == c.bounds[0] for x in c.calls[0][1]), exact=False))
    hv = HIST_VALUES
    cs.append(_agg("digit_edges/one_series_each", HISTOGRAM, len(hv), [(np.arange(len(hv)), hv, NOBAD, 0)], DEFAULT_BOUNDS, exact=True,
                   pred=lambda c: {(((f2b(abs(b2f(x))) >> 52) or 1) - 1) & 31 for x in c.calls[0][1] if math.isfinite(b2f(x)) and b2f(x)} >= {0, 1, 31}))
    fin = [x for x in hv if math.isfinite(x)]
    cs.append(_agg("digit_edges/all_in_one_series", HISTOGRAM, 1, [(np.zeros(len(fin)), fin, NOBAD, 0)], DEFAULT_BOUNDS, exact=False,
                   pred=lambda c: True))
    for name, vals in (("pinf_alone", [1.0, math.inf, 2.0]), ("ninf_alone", [1.0, -math.inf]), ("pinf_with_ninf", [math.inf, 1.0, -math.inf]), ("nan", [1.0, math.nan, math.inf])):
        cs.append(_agg("specials/" + name, HISTOGRAM, 1, [(np.zeros(len(vals)), vals, NOBAD, 0)], DEFAULT_BOUNDS, pred=lambda c: True))
    # ---- chains: the running sum's sign across calls (k_l2m_normalize's signed carry) and the rounding of what they end on
    T = math.ldexp(1.0, 200)
    chains = {
        "pos_neg_zero_pos": [[3.0, T], [-T, -T, -8.0], [T, 5.0], [0.25]],
        "neg_small_from_large": [[-T], [T, -5e-324], [5e-324], [-DBL_MAX, DBL_MAX, 5e-324]],
        "tie_to_even_down": [[1.0], [math.ldexp(1.0, -53)], [0.0]],                                   # 1 + 2^-53: tie, even below
        "tie_to_even_up": [[1.0, math.ldexp(1.0, -52)], [math.ldexp(1.0, -53)], [0.0]],               # 1 + 2^-52 + 2^-53: tie, even above
        "sticky_60_limbs_below": [[math.ldexp(1.0, 32 * 61 - 1074)], [math.ldexp(1.0, 32 * 61 - 1074 - 53)], [5e-324]],   # tie broken by one ulp of the smallest digit
        "sticky_negative": [[-math.ldexp(1.0, 32 * 61 - 1074)], [-math.ldexp(1.0, 32 * 61 - 1074 - 53)], [-5e-324]],
        "subnormal_result": [[math.ldexp(1.0, -1022)], [-math.ldexp(1.0, -1023), 5e-324], [-1e-310]],
        "smallest_subnormals_add_up": [[5e-324] * 3, [5e-324, -5e-324], [5e-324] * 4],
        "twice_dbl_max": [[DBL_MAX], [DBL_MAX], [0.0]],
        "overflow_then_back": [[DBL_MAX, DBL_MAX], [DBL_MAX], [-DBL_MAX, -DBL_MAX, -DBL_MAX, 1.0]],
        "negative_overflow": [[-DBL_MAX], [-DBL_MAX, -DBL_MAX], [-DBL_MAX]],
        "just_under_the_rounding_overflow": [[DBL_MAX], [math.ldexp(1.0, 969)], [0.0]],                 # 2^1024 - 2^971 + 2^969: rounds back to DBL_MAX
        "exactly_the_rounding_overflow": [[DBL_MAX], [math.ldexp(1.0, 970)], [0.0]],                    # 2^1024 - 2^970: the tie, up to +inf
        "exactly_the_rounding_overflow_negative": [[-DBL_MAX], [-math.ldexp(1.0, 970)], [0.0]],
        "top_digit_many_dbl_max": [[DBL_MAX] * 200, [DBL_MAX] * 56, [-DBL_MAX] * 255],
    }
    for name, calls in chains.items():
        cc, base = [], 0
        for vals in calls:
            cc.append((np.zeros(len(vals)), vals, NOBAD, base)); base += len(vals)
        cs.append(_agg("chain/" + name, HISTOGRAM, 1, cc, DEFAULT_BOUNDS, pred=lambda c: len(c.calls) >= 3, exact=False))
    return cs


def chain_sign_walk(c):
    """the signs of the running sum after each call of a chain case"""
    m = AggModel(c.mode, c.nseries, c.bounds)
    out = []
    for sid, val, fb, base in c.calls:
        m.call(sid, val, fb, base)
        out.append((m.sum[0] > 0) - (m.sum[0] < 0))
    return out


def gauge_later_range_case():
    """a merged row whose last index lies BEHIND this call's range (another rank's records): idx_base + n + 1, one past what the
    hand-over may read.  The series keeps its value."""
    rows = np.zeros((2, row_words(GAUGE)), dtype=np.uint64)
    rows[1, L2M_W_FIRST] = (~5) & M64
    rows[1, L2M_W_LASTIDX] = 1000 + 4 + 1
    rows[1, L2M_W_LASTVAL] = f2b(7.25)
    return Case("agg/gauge/untouched_series_with_a_later_index", lambda c: int(c.rows[1, L2M_W_LASTIDX]) - 1 - c.idx_base == len(c.sid),
                mode=GAUGE, rows=rows, sid=np.array([0, 0, NONE, 0], dtype=np.uint32), val=np.array([1.0, 2.0, 3.0, 4.0]).view(np.uint64), idx_base=1000)


# ------------------------------------------------------------------------------------------ column cases as records, for the oracle
def as_records(c):
    """an aggregate case as chunks for oracle_binding.L2M: label k = the series id, value_field v; NONE / DEFER rows make no observation,
    a stale-flagged row is skipped likewise (the aggregation skips the flag; the stale scan's cases have records of their own), a call
    cut by first_bad gets a byte that is no msgpack"""
    chunks = []
    for sid, val, fb, base in c.calls:
        recs = []
        for i in range(len(sid)):
            if i == fb:
                recs.append(b"\xc1")
            s = int(sid[i])
            if s >= STALE:
                recs.append(mp(1) if c.mode == COUNTER else v2_record(1, 0, {"k": "x"}))
            else:
                body = {"k": "s%d" % s}
                if c.mode != COUNTER: body["v"] = b2f(val[i])
                recs.append(v2_record(1, 0, body))
        chunks.append(b"".join(recs))
    return chunks


def stale_as_records(c):
    """a stale case as one gauge chunk with a series per row: row i's value ends up as series r<i>'s"""
    recs = []
    for i in range(c.n):
        if i == c.first_bad:
            recs.append(b"\xc1")
        s = int(c.sid[i])
        if s in (NONE, DEFER): recs.append(v2_record(1, 0, {"k": "r%d" % i}))
        elif s & STALE: recs.append(v2_record(1, 0, {"k": "r%d" % i, "v": "zzz"}))
        else: recs.append(v2_record(1, 0, {"k": "r%d" % i, "v": b2f(c.val[i])}))
    return b"".join(recs)


# ------------------------------------------------------------------------------------------ record cases: k_l2m_extract
X_PROPS = [("add_label", "x $m['x']")]          # a nested name: k_l2m_extract, not k_l2m_lane


def xrec(size, label="a", v=None):
    """a record of exactly `size` bytes: {"m": {"x": label}, ["v": v,] ["p": padding]} -- the padding string always has the three-byte
    str16 header, so every size from the bare record + 5 up can be made (48 bytes and up for a label of up to 8 characters)"""
    body = {"m": {"x": label}}
    if v is not None: body["v"] = v
    bare = v2_record(1, 0, body)
    if size == len(bare): return bare
    pad = size - len(bare) - 5
    assert pad >= 0, (size, len(bare))
    body["p"] = Raw(b"\xda" + struct.pack(">H", pad) + b"p" * pad)
    r = v2_record(1, 0, body)
    assert len(r) == size
    return r


def stage_plan(lens, n_waves=None):
    """k_l2m_extract's staging of a chunk whose records have the lengths `lens`: per wave of 64 rows, [(first lane, records, direct,
    bytes with align)] -- the kernel's while (lo < cnt) loop"""
    off = np.concatenate([[0], np.cumsum(lens)])
    plan = []
    for base in range(0, len(lens), 64):
        cnt, lo, st = min(64, len(lens) - base), 0, []
        while lo < cnt:
            g0 = int(off[base + lo]); align = g0 & 15
            m = 0
            while lo + m < cnt and int(off[base + lo + m + 1]) - g0 + align <= L2M_TILE: m += 1
            if m == 0: st.append((lo, 1, True, int(off[base + lo + 1]) - g0 + align)); lo += 1
            else: st.append((lo, m, False, int(off[base + lo + m]) - g0 + align)); lo += m
        plan.append(st)
    return plan


def _xcase(name, recs, pred, mode="counter", **kw):
    return Case("extract/" + name, pred, recs=recs, data=b"".join(recs), mode=mode, props=X_PROPS, **kw)


def _filler(align, tag):
    """64 records (one wave) whose bytes end on `align` mod 16"""
    recs = [xrec(48, "f%d" % (i % 3), float(i)) for i in range(63)] + [xrec(48 + align, tag, 1.0)]
    assert sum(map(len, recs)) % 16 == align
    return recs


def extract_fit_cases():
    cs = []
    for align in range(16):
        for d, what in ((0, "exact"), (1, "one_over"), (-1, "one_under")):
            total = L2M_TILE - align + d
            wave = [xrec(288, "w%d" % (i % 5), float(i) - 7.5) for i in range(63)]
            wave.append(xrec(total - 63 * 288, "last%d" % align, 0.5))
            recs = _filler(align, "fill") + wave
            want = [(0, 64, False, L2M_TILE + d)] if d <= 0 else [(0, 63, False, 63 * 288 + align), (63, 1, False, total - 63 * 288 + (63 * 288 + 3072 + align) % 16)]
            cs.append(_xcase("fit/align=%d/%s" % (align, what), recs, lambda c, want=want: stage_plan([len(r) for r in c.recs])[1] == want, mode="histogram"))
    return cs


def extract_single_cases():
    cs = []
    small = lambda i: xrec(48 + i % 7, "s%d" % (i % 4), float(i))
    for align in (0, 1, 15):
        for d, direct in ((0, False), (1, True)):
            big = xrec(L2M_TILE - align + d, "big", 2.5)
            recs = _filler(align, "fill") + [big, small(1), small(2)]
            cs.append(_xcase("single/align=%d/%s" % (align, "read_in_place" if direct else "fills_the_tile"), recs, mode="histogram",
                             pred=lambda c, direct=direct: stage_plan([len(r) for r in c.recs])[1][0][1:] == (1, direct, L2M_TILE + int(direct))))
    for lanes in ([0], [31], [63], [20, 21], [0, 63], [62, 63]):
        recs = [small(i) for i in range(64 + 5)]
        for k, l in enumerate(lanes):
            recs[l] = xrec(L2M_TILE + 17 + 100 * k, "over%d" % l, 1.25)
        cs.append(_xcase("single/over_the_tile_at_lane_" + "_".join(map(str, lanes)), recs, mode="histogram",
                         pred=lambda c, lanes=lanes: [s[0] for s in stage_plan([len(r) for r in c.recs])[0] if s[2]] == lanes
                         and sum(s[1] for s in stage_plan([len(r) for r in c.recs])[0]) == 64))
    return cs


def extract_end_cases():
    cs = []
    for r in range(16):
        recs = [xrec(48, "a", 1.0), xrec(57, "b", 2.0)]
        recs.append(xrec(48 + (r - 153) % 16, "end%d" % r, 3.0))
        cs.append(_xcase("chunk_end/residue=%d" % r, recs, lambda c, r=r: len(c.data) % 16 == r and len(c.data) > 16, mode="gauge"))
    return cs


def extract_count_cases():
    cs = []
    for n in (1, 63, 64, 65, 255, 256, 257):
        recs = [xrec(48 + i % 5, "c%d" % (i % 6), float(i)) for i in range(n)]
        cs.append(_xcase("rows=%d" % n, recs, lambda c, n=n: len(c.recs) == n, mode="histogram"))
    return cs


def second_trip_rows(cus, extra=65):
    """2 x CUs x 256 + 65 rows of 21 to 24 bytes for a counter; the rows of the second trip carry a label seen nowhere else"""
    first = 2 * cus * L2M_BLOCK
    kinds = [v2_record(1, 0, {"m": {"x": l}}) for l in ("a", "bb", "ccc", "dddd")]
    recs = [kinds[(i * 7) % 4] for i in range(first)] + [v2_record(1, 0, {"m": {"x": "2nd"}})] * extra
    return _xcase("second_trip/cus=%d" % cus, recs, lambda c: len(c.recs) == first + extra and all(21 <= len(r) <= 24 for r in c.recs[::997])
                  and c.recs[first] not in c.recs[:first:101], first=first)


class RowChunk(bytes):
    """a chunk that is handed over as a device chunk with these rows (empty rows included); its bytes are what the oracle reads"""
    rows = ()


def row_chunk(rows):
    c = RowChunk(b"".join(rows))
    c.rows = list(rows)
    return c


BAD = b"\xc1"                                     # never a msgpack type byte: msgpack_unpack_next stops the callback's loop there


def extract_dev_cases(cus):
    """device chunks: empty rows (records an earlier filter dropped) between full ones, a row that does not decode at the wave and
    workgroup edges and at the first row of the second trip; a good call follows each"""
    cs = []
    good = row_chunk([xrec(48, "g", 1.0), xrec(49, "h", 2.0)])
    rec = lambda i: xrec(48 + i % 3, "d%d" % (i % 5), float(i))
    rows = [rec(i) if i % 3 else b"" for i in range(200)]
    cs.append(Case("extract/dev/empty_rows", lambda c: c.chunks[0].rows.count(b"") > 60 and c.chunks[0].rows[0] == b"" and c.chunks[0].rows[64] != b"",
                   chunks=[row_chunk(rows), good, row_chunk([b"", b""]), good], mode="histogram", props=X_PROPS))
    for at in (63, 64, 255, 256, 2 * cus * L2M_BLOCK):
        n = at + 70
        if at < 1000:
            rows = [rec(i) for i in range(n)]
        else:
            kinds = [rec(i) for i in range(15)]
            rows = [kinds[(i * 7) % 15] for i in range(n)]
        rows[at] = BAD
        rows[at + 3] = xrec(50, "never", 1.0)
        if at > 10: rows[at - 2] = b""
        cs.append(Case("extract/dev/undecodable_row_%d%s" % (at, "" if at < 1000 else "_second_trip"), lambda c, at=at: c.chunks[0].rows[at] == BAD and len(c.chunks[0].rows) > at + 64,
                       chunks=[row_chunk(rows), good], mode="gauge" if at == 64 else "histogram", props=X_PROPS))
    return cs


def generic_case():
    """4096 x 64 + 64 records whose label is a float (each defers to k_l2m_generic, whose grid is 4096 x 64 lanes: the last 64 are its
    second trip) -- those carry a label value seen nowhere else"""
    first = L2M_GENERIC_GRID * 64
    a, b, z = (v2_record(1, 0, {"a": x}) for x in (1.5, -0.25, 2.5))
    recs = [a if (i * 5) % 3 else b for i in range(first)] + [z] * 64
    return Case("generic/second_trip", lambda c: len(c.recs) == first + 64 and set(c.recs[first:]) == {z} and z not in set(c.recs[:first]),
                recs=recs, data=b"".join(recs), mode="counter", props=[("label_field", "a")], first=first)


# ------------------------------------------------------------------------------------------ the dictionary
def l2m_mix(h):
    h ^= h >> 32; h = (h * 0x9E3779B97F4A7C15) & M64; h ^= h >> 29; h = (h * 0xBF58476D1CE4E5B9) & M64; h ^= h >> 32
    return h + 2 if h < 2 else h


def key_hash(labels):
    """l2m_series_id_lv: FNV-1a over the label tuple's byte stream (each label's bytes, then NUL), mixed"""
    h = 0xcbf29ce484222325
    for l in labels:
        for b in l + b"\0":
            h = ((h ^ b) * 0x100000001b3) & M64
    return l2m_mix(h)


def home_slot(label, cap):
    return key_hash([label]) & (cap - 1)


def wrap_keys(cap=16, top=2):
    """key names for the cap-16 sweep: the first `top` have the LAST slot as their home, so one of them must wrap to slot 0 whatever
    the order the lanes arrive in; the others follow in name order"""
    names = [b"k%d" % i for i in range(400)]
    last = [k for k in names if home_slot(k, cap) == cap - 1][:top]
    rest = [k for k in names if k not in last]
    return last + rest


def padded(label):
    return (len(label) + 1 + 7) & ~7
