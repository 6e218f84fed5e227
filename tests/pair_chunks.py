"""The named chunks of the fused [filter_parser, filter_grep] tests, kept apart so that they can be built and looked at without a
device.  Every chunk is deterministic and built from lengths; each group aims at one family of edges of k_pg_decide / k_pg_emit
(csrc/fused_kernels.inc) and of the helpers they call (csrc/kdev.inc LdsSink, pg_rule_match).  tests/test_pair_chunks.py asserts on
the CPU oracle, with the small model of the emit kernel's batching rule below, that each chunk still reaches the edge it is named
for; tests/test_pair_emit_gpu.py runs them on the device.  The model is never used to compute expected bytes.

group(name) -> [Chunk]; a Chunk carries its records, the parser's arguments, the rules and a short name."""
import functools

APACHE2 = (r'^(?<host>[^ ]*) [^ ]* (?<user>[^ ]*) \[(?<time>[^\]]*)\] "(?<method>\S+)(?: +(?<path>[^ ]*) +\S*)?" '
           r'(?<code>[^ ]*) (?<size>[^ ]*)(?: "(?<referer>[^\"]*)" "(?<agent>.*)")?$')
TF = "%d/%b/%Y:%H:%M:%S %z"
TIME_LAST = r'^(?<code>[^ ]*) (?<msg>[^\[]*)\[(?<time>[^\]]*)\](?<t>.*)$'      # the time text is the last thing of a short line
TWO_FIELDS = r'^(?<code>\d+) (?<m>.*)$'                                         # no time key: records stay under 100 bytes
P_APACHE = dict(regex=APACHE2, time_fmt=TF, time_key="time")
P_TIME_LAST = dict(regex=TIME_LAST, time_fmt=TF, time_key="time")
P_TWO = dict(regex=TWO_FIELDS)
KEEP_5XX = (("regex", r"code ^5\d\d$"),)
TIME_TEXT = b"10/Mar/2024:08:34:03 +0900"

# ---- the constants of k_pg_emit the chunks are laid out for (csrc/fused_kernels.inc: PGE_ROWS, PGE_STG_PLAIN, PGE_STG_GENERAL; the
# group of 64 is the wave; a workgroup of four waves takes 2048 rows).  Whoever changes one of them there moves it here too: the
# coverage asserts of tests/test_pair_chunks.py then say which chunks no longer sit on their edge.
PGE_ROWS = 512
PGE_GROUP = 64
PGE_WORKGROUP_ROWS = 4 * PGE_ROWS
PGE_STG_PLAIN = 8192
PGE_STG_GENERAL = 9728
REG_WINDOW = 272                 # bytes of a value the single pass holds in registers; the rest comes through 64-byte windows (tile_kernels.inc k_parser_reg)
RULE_LDS_ROOM = 48 * 1024        # k_pg_decide stages the rules' tables in LDS up to here (flbgpu.cpp run_pair_fused)
GROUPS = ("staging", "one_big", "full_batch", "queue", "tails", "time_end", "fields", "values", "rules")


class Chunk:
    def __init__(self, name, recs, pargs, rules=KEEP_5XX, op=None, tail=b"", **notes):
        self.name, self.recs, self.pargs, self.rules, self.op, self.tail, self.notes = name, list(recs), dict(pargs), list(rules), op, tail, notes

    @property
    def blob(self):
        return b"".join(self.recs)

    def __repr__(self):
        return "Chunk(%s, %d records)" % (self.name, len(self.recs))


# ---- msgpack by hand (the layout filter_parser writes and in_* plugins deliver)
def str_hdr(n):
    return bytes([0xa0 | n]) if n < 32 else b"\xd9" + bytes([n]) if n < 256 else b"\xda" + n.to_bytes(2, "big") if n < 65536 else b"\xdb" + n.to_bytes(4, "big")


def mp_str(b):
    return str_hdr(len(b)) + b


def mp_map(d):
    assert len(d) < 16
    return bytes([0x80 | len(d)]) + b"".join(mp_str(k) + mp_str(v) for k, v in d.items())


def record(line, row=0, meta=None):
    """a v2 log event {"log": line}: [[ext time, metadata], body]"""
    return b"\x92\x92\xd7\x00" + (1700000000 + row).to_bytes(4, "big") + (row % 1000).to_bytes(4, "big") + mp_map(meta or {}) + mp_map({b"log": line})


def value_len(rec):
    """bytes of the "log" value of a record() without metadata"""
    t = rec[18]
    return t & 31 if t < 0xc0 else rec[19] if t == 0xd9 else int.from_bytes(rec[19:21], "big") if t == 0xda else int.from_bytes(rec[19:23], "big")


def apache_line(code=503, agent=b"", path=b"/p", referer=b"-", host=b"10.0.0.1", time=TIME_TEXT, size=b"17"):
    """LINE_BASE bytes + the agent (with the defaults)"""
    return host + b" - - [" + time + b'] "GET ' + path + b' HTTP/1.1" ' + (b"%d" % code) + b" " + size + b' "' + referer + b'" "' + agent + b'"'


LINE_BASE = len(apache_line())


def parsed_size(fields, meta_len=1):
    """bytes of the record filter_parser writes for these named fields (empty ones are skipped): 92 92 d7 00 + 8, the metadata, a
    fixmap header, the keys and values as strings.  Used to LAY OUT a chunk; what the sizes really are comes from the oracle."""
    kept = [(k, v) for k, v in fields if v]
    assert len(kept) < 16
    return 12 + meta_len + 1 + sum(len(mp_str(k)) + len(mp_str(v)) for k, v in kept)


def apache_size(agent_len, path_len=2, referer_len=1, host_len=8, size_len=2):
    f = [(b"host", b"h" * host_len), (b"user", b"-"), (b"method", b"GET"), (b"path", b"p" * path_len), (b"code", b"503"), (b"size", b"s" * size_len),
         (b"referer", b"r" * referer_len), (b"agent", b"a" * agent_len)]
    return parsed_size(f)


def agent_for_size(size, lo=1, hi=70000):
    """the agent length whose kept record has `size` bytes (None at the two str-header steps)"""
    for hdr in (1, 2, 3, 5):
        n = size - apache_size(1) + 2 - hdr
        if lo <= n <= hi and apache_size(n) == size:
            return n
    return None


# ---- the batching rule of k_pg_emit as a model: which batches a wave forms from the kept rows' output sizes
class Batch:
    def __init__(self, wave, group, lo, rows, direct, align, end, next_end):
        self.wave, self.group, self.lo, self.rows, self.direct, self.align, self.end, self.next_end = wave, group, lo, rows, direct, align, end, next_end

    def __repr__(self):
        return "Batch(wave %d group %d lane %d: %d rows, align %d, end %d, next %s%s)" % (
            self.wave, self.group, self.lo, len(self.rows), self.align, self.end, self.next_end, ", direct" if self.direct else "")


def wave_kept(keep_len):
    """kept rows of every wave's window of PGE_ROWS rows"""
    return [sum(1 for x in keep_len[b:b + PGE_ROWS] if x) for b in range(0, len(keep_len), PGE_ROWS)]


def batches(keep_len, stg):
    """keep_len[r] = output bytes of input row r (0: dropped).  A wave queues the kept rows of its PGE_ROWS rows, takes them 64 at a
    time and forms greedy batches: records are added while o1 - batch_base + (batch_base & 15) <= stg; a record that does not fit an
    empty batch goes alone and straight to global memory (`direct`).  end / next_end: that sum for the batch's last record and for
    the record behind it in the group (None: the group ends)."""
    off = [0]
    for x in keep_len:
        off.append(off[-1] + x)
    out = []
    for base in range(0, len(keep_len), PGE_ROWS):
        q = [r for r in range(base, min(len(keep_len), base + PGE_ROWS)) if keep_len[r]]
        for k0 in range(0, len(q), PGE_GROUP):
            grp = q[k0:k0 + PGE_GROUP]
            lo = 0
            while lo < len(grp):
                bb = off[grp[lo]]
                align = bb & 15
                m = 0
                while lo + m < len(grp) and off[grp[lo + m] + 1] - bb + align <= stg:
                    m += 1
                direct = m == 0
                if direct:
                    m = 1
                nxt = off[grp[lo + m] + 1] - bb + align if lo + m < len(grp) else None
                out.append(Batch(base // PGE_ROWS, k0 // PGE_GROUP, lo, grp[lo:lo + m], direct, align, off[grp[lo + m - 1] + 1] - bb + align, nxt))
                lo += m
    return out


# ---- (a) staging sweep: a batch that ends at STG - 1, STG, or whose next record would end at STG + 1, from every alignment
SMALL_AGENT, FILL_AGENT = 20, 190


def staging_chunk(stg, first_agent, delta):
    """rows 0 .. 63: one group of short kept records in one batch, the first with an agent of first_agent bytes -- the second group
    starts where that batch ends, at every alignment as first_agent grows.  Rows 64 ..: records of a 263-byte value and two adjustable
    records after which the sum (alignment included) is stg + delta; a kept record of another fill byte behind it, a dropped one last.
    Every value has at most REG_WINDOW bytes; every kept record with an agent carries a descriptor (an empty agent is the generic kernel's)."""
    sizes = [apache_size(first_agent)] + [apache_size(SMALL_AGENT)] * (PGE_GROUP - 1)
    assert sum(sizes) <= PGE_STG_PLAIN
    recs = [apache_line(agent=b"h" * first_agent)] + [apache_line(agent=b"f" * SMALL_AGENT)] * (PGE_GROUP - 1)
    target = stg - (sum(sizes) & 15) + delta
    big = apache_size(FILL_AGENT)
    lo, hi = apache_size(32), apache_size(REG_WINDOW - LINE_BASE)
    count = (target - 2 * lo) // big
    rest = target - count * big
    adj = [agent_for_size(x, 32, REG_WINDOW - LINE_BASE) for x in ((rest - lo, lo) if rest - lo <= hi else (hi, rest - hi))]
    assert None not in adj and count + 4 <= PGE_GROUP
    recs += [apache_line(agent=b"b" * FILL_AGENT)] * count + [apache_line(agent=b"j" * adj[0]), apache_line(agent=b"k" * adj[1])]
    recs += [apache_line(agent=b"N" * 40), apache_line(code=200, agent=b"d" * 9)]
    assert all(len(r) <= REG_WINDOW for r in recs)
    return Chunk("staging %d, first agent %d, %+d" % (stg, first_agent, delta), [record(r, i) for i, r in enumerate(recs)], P_APACHE,
                 stg=stg, first_agent=first_agent, delta=delta)


def staging_chunks():
    return [staging_chunk(stg, k, d) for stg in (PGE_STG_PLAIN, PGE_STG_GENERAL) for k in range(32) for d in (-1, 0, 1)]


# ---- (b) one record around the staging size, behind a short kept record that sets its alignment
def one_big_chunk(stg, align, delta):
    small = next(n for n in range(1, 32) if apache_size(n) & 15 == align)
    big = agent_for_size(stg - align + delta)
    assert big is not None and big + LINE_BASE > REG_WINDOW
    lines = [apache_line(agent=b"s" * small), apache_line(agent=b"B" * big), apache_line(code=200, agent=b"d" * 5), apache_line(agent=b"N" * 33),
             apache_line(code=301, agent=b"d" * 6)]
    return Chunk("one record of %d %+d bytes at align %d" % (stg, delta, align), [record(r, i) for i, r in enumerate(lines)], P_APACHE,
                 stg=stg, align=align, delta=delta)


def direct_between_staged():
    lines = [apache_line(agent=b"s" * (5 + i)) for i in range(5)] + [apache_line(agent=b"B" * (PGE_STG_GENERAL + 100))]
    lines += [apache_line(agent=b"t" * (35 + i)) for i in range(5)] + [apache_line(code=200, agent=b"d")]
    return Chunk("direct record between staged ones", [record(r, i) for i, r in enumerate(lines)], P_APACHE)


def one_big_chunks():
    return [one_big_chunk(stg, a, d) for stg in (PGE_STG_GENERAL, PGE_STG_PLAIN) for a in range(16) for d in (-1, 0, 1)] + [direct_between_staged()]


# ---- (c) a whole group of 64 queued records in one batch
def full_batch_chunks():
    out = []
    for pargs, mk, what in ((P_TWO, lambda i: b"503 " + b"m" * (1 + i % 50), "two fields"),
                            (P_TIME_LAST, lambda i: b"503 " + b"m" * (1 + i % 9) + b" [" + TIME_TEXT + b"]" + b"t" * (i % 7), "time last")):
        for kept in (64, 65, 128):
            lines = [mk(i) for i in range(kept)] + [b"200 dropped" if pargs is P_TWO else b"200 dropped [" + TIME_TEXT + b"]x"]
            out.append(Chunk("%d kept in a row, %s" % (kept, what), [record(r, i) for i, r in enumerate(lines)], pargs, kept=kept))
    return out


# ---- (d) queue seams: kept counts per wave, kept rows at the wave and workgroup seams, the r < n guard
QUEUE_N = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)
WINDOW_KINDS = ("only row 0", "only row 63", "only row 64", "only row 511", "rows 0..63", "rows 1..63", "rows 0..64", "none", "all", "none")
SEAM_ROWS = (0, 63, 64, 511, 512, 2047, 2048)


def _window_keeps(kind, i):
    return {"only row 0": i == 0, "only row 63": i == 63, "only row 64": i == 64, "only row 511": i == 511, "rows 0..63": i < 64,
            "rows 1..63": 1 <= i < 64, "rows 0..64": i < 65, "none": False, "all": True}[kind]


def queue_patterns(n):
    """name -> the kept rows; window w of the `shift s` patterns has kind (w + s) of WINDOW_KINDS (all -> none and none -> all follow
    each other there)"""
    pats = {}
    shifts = range(len(WINDOW_KINDS)) if n <= 513 else (0, 3, 7)
    for s in shifts:
        pats["shift %d" % s] = [r for r in range(n) if _window_keeps(WINDOW_KINDS[(r // PGE_ROWS + s) % len(WINDOW_KINDS)], r % PGE_ROWS)]
    pats["only the last row"] = [n - 1]
    pats["the seam rows and the last"] = sorted(set([r for r in SEAM_ROWS if r < n] + [n - 1]))
    pats["all but row 0"] = list(range(1, n))
    return pats


def queue_chunk(n, name, kept):
    ks = set(kept)
    lines = [apache_line(code=503 if r in ks else 200, agent=b"q" * (1 + r % 29), size=b"%d" % r) for r in range(n)]
    return Chunk("queue n=%d, %s" % (n, name), [record(ln, r) for r, ln in enumerate(lines)], P_APACHE, n=n, kept=sorted(ks), pattern=name)


def queue_chunks():
    """(the patterns that keep nothing or everything are another path -- the pair hands such a chunk to the unfused kernels -- and
    are left out; n = 1 with its record kept is the one named exception: unfused_queue_chunk)"""
    out = []
    for n in QUEUE_N:
        seen = set()
        for name, kept in queue_patterns(n).items():
            if 0 < len(kept) < n and tuple(kept) not in seen:
                seen.add(tuple(kept))
                out.append(queue_chunk(n, name, kept))
    return out


def unfused_queue_chunk():
    return queue_chunk(1, "its one record kept (grep answers NOTOUCH)", [0])


# ---- (e) last-field tails: the agent is the last field written; 16-byte tail copies must stop at the record's end
TAIL_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48)
GARBAGE = b"\x92\x92\xd7\x00"          # the start of an event that never ends: the decoder stops there


def tail_chunks():
    out = []
    for ll in TAIL_LENGTHS:
        a = apache_line(agent=b"T" * ll)
        nb = apache_line(agent=b"Z" * 21)                                                     # the neighbour, another fill byte
        drop = apache_line(code=200, agent=b"d" * 7)
        head = [apache_line(agent=b"f" * (2 + i % 11)) for i in range(PGE_GROUP - 1)] + [a, nb, drop, nb, a, nb, drop]     # `a` at lane 63: last of its batch
        for ending, last in (("last record of the chunk", [drop, a]), ("last kept record of the chunk", [a, drop])):
            for tail in (b"", GARBAGE):
                lines = head + last
                out.append(Chunk("agent of %d bytes, %s%s" % (ll, ending, ", bytes behind it" if tail else ""), [record(r, i) for i, r in enumerate(lines)],
                                 P_APACHE, tail=tail, agent=ll, lane63=PGE_GROUP - 1))
    return out


# ---- (f) the time text at the chunk's end: pge_time reads 32 bytes, or what is left of the chunk
TIME_END_AFTER = (1, 2, 5, 6, 7, 22)                    # bytes between the end of the time text and the end of the chunk
ODD_TIMES = (b"10/Foo/2024:08:34:03 +0900", b"5/March/2024:8:34:03 +0900")       # the plan's length, not its layout: reported, the call repeated


def time_end_chunks():
    out = []
    for after in TIME_END_AFTER:
        for text in (TIME_TEXT,) + ODD_TIMES:
            lines = [b"%d row %d [" % (503 if i % 3 == 0 else 200, i) + TIME_TEXT + b"]" + b"t" * (i % 5) for i in range(40)]
            lines.append(b"503 the last one [" + text + b"]" + b"e" * (after - 1))
            out.append(Chunk("chunk ends %d bytes behind %s" % (after, "its time text" if text is TIME_TEXT else text.decode()),
                             [record(r, i) for i, r in enumerate(lines)], P_TIME_LAST, after=after, odd=text is not TIME_TEXT, left=len(text) + after))
    # the same odd text in a kept record far from the chunk's end: reported by the emit pass, the call repeated
    lines = [b"%d row %d [" % (503 if i % 3 == 0 else 200, i) + (ODD_TIMES[0] if i == 3 else TIME_TEXT) + b"]" + b"t" * (i % 5) for i in range(400)]
    out.append(Chunk("odd time text in a kept record in the middle", [record(r, i) for i, r in enumerate(lines)], P_TIME_LAST, odd=True, middle=True))
    return out


# ---- (g) parsers of 1 .. 31 named groups (the regex compiler takes 31 capture groups; a 32nd is refused when the parser is made)
FIELD_COUNTS = (1, 2, 3, 8, 9, 10, 15, 16, 17, 31)
REFUSED_FIELD_COUNTS = (32, 33)
# `[^ ]*` fields: from 14 of them on the capture automaton passes the table compiler's state budget, the parser runs on the NFA engine and
# the pair is not fused (flbgpu.cpp pair_fusable) -- those counts run unfused, against the same oracle
UNFUSED_FIELD_COUNTS = (15, 16, 17, 31)


def fields_regex(nf, cls="[a-z0-9]"):
    return "^" + " ".join("(?<f%d>%s*)" % (i, cls) for i in range(nf)) + "$"


def fields_chunks():
    out = []
    for nf, cls in [(n, "[a-z0-9]") for n in FIELD_COUNTS] + [(n, "[^ ]") for n in UNFUSED_FIELD_COUNTS]:
        lines = [b" ".join([b"" if i % 4 == 1 and (i + f) % 5 == 0 else b"v%d" % (i * 7 + f) for f in range(nf - 1)] + [b"k%d" % i if i % 3 == 0 else b"x%d" % i]) for i in range(200)]
        out.append(Chunk("%d fields of %s*" % (nf, cls), [record(r, i) for i, r in enumerate(lines)], dict(regex=fields_regex(nf, cls)), [("regex", "f%d ^k" % (nf - 1))],
                         nf=nf, unfused=cls == "[^ ]"))
    # a kept record with metadata: the 9-field parser (apache2) and the 2-field one
    for pargs, kept, drop, what in ((P_APACHE, apache_line(agent=b"m" * 12), apache_line(code=200, agent=b"m" * 12), "9 fields"),
                                    (P_TWO, b"503 with metadata", b"200 with metadata", "2 fields")):
        recs = [record(kept if i % 3 == 0 else drop, i, meta={b"k": b"v"} if i in (3, 4, 9) else None) for i in range(12)]
        out.append(Chunk("metadata, " + what, recs, pargs, meta_rows=(3, 4, 9)))
    return out


# ---- (h) value lengths: the single pass's register window, and 0xFFFF
def value_chunks():
    lines = []
    for v in range(REG_WINDOW - 4, REG_WINDOW + 5):
        lines += [apache_line(agent=b"w" * (v - LINE_BASE)), apache_line(code=200, agent=b"d" * (v - LINE_BASE))]
    assert [len(x) for x in lines[::2]] == list(range(268, 277))
    out = [Chunk("kept values of 268..276 bytes", [record(r, i) for i, r in enumerate(lines)], P_APACHE, lengths=list(range(268, 277)))]
    lines = [apache_line(agent=b"o" * 11)]
    for v in (65534, 65535, 65536):
        lines += [apache_line(agent=b"V" * (v - LINE_BASE)), apache_line(agent=b"o" * (v % 13))]
    lines.append(apache_line(code=200, agent=b"d" * 3))
    out.append(Chunk("kept values of 65534..65536 bytes", [record(r, i) for i, r in enumerate(lines)], P_APACHE, lengths=[65534, 65535, 65536]))
    return out


# ---- (i) rules k_pg_decide evaluates: the register DFA up to 16 bytes, dfa_match beyond; tables in LDS and in global memory
RULE_FIELD_LENGTHS = (0, 1, 15, 16, 17, 32)
# tables of (a|b)*a(a|b){k}: 2^(k+1) states and a few; measured with flbgpu_rx_info (classes x states -> 256 + 2 * classes * states + states bytes):
#   agent (a|b)*a(a|b){10}[YZ]$   6 x 2052 -> 26 932 bytes   staged in LDS
#   agent (a|b)*a(a|b){10}Z$      6 x 2052 -> 26 932 bytes   53 876 with the first: past the room, walked in global memory
#   agent (a|b)*b(a|b){8}[YZ]$    6 x 516  ->  6 964 bytes   fits behind the first: staged in LDS again
BIG_TABLE_RULES = (("regex", r"agent (a|b)*a(a|b){10}[YZ]$"), ("regex", r"agent (a|b)*a(a|b){10}Z$"), ("regex", r"agent (a|b)*b(a|b){8}[YZ]$"))


def _rule_lines(hi_byte):
    lines = []
    for ll in RULE_FIELD_LENGTHS:
        for last in (b"Z", b"Y"):
            agent = (b"q" * (ll - 1) + last) if ll else b""
            lines.append(apache_line(agent=agent, referer=b"caf\xc3\xa9" if hi_byte else b"-"))
    return lines


def _ab(seed, n):
    out, x = bytearray(), seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(b"ab"[(x >> 16) & 1])
    return bytes(out)


def rules_chunks():
    out = []
    keep_time = dict(P_APACHE, time_keep=True)
    sets = (("OR", [("regex", "time ^99"), ("regex", "agent Z$")]), ("AND", [("regex", "time 2024"), ("regex", "agent Z$")]),
            (None, [("exclude", "time ^99"), ("regex", "agent Z$")]))
    for op, rules in sets:
        out.append(Chunk("Z$ with a rule on the kept time, %s" % (op or "legacy"), [record(r, i) for i, r in enumerate(_rule_lines(False))], keep_time, rules, op, decide=True))
    for op, rules in ((None, [("regex", "agent Z$")]), ("AND", [("regex", "agent Z$"), ("regex", "code ^5")])):
        out.append(Chunk("Z$ on records with a byte >= 0x80 elsewhere, %s" % (op or "legacy"), [record(r, i) for i, r in enumerate(_rule_lines(True))], P_APACHE, rules, op, decide=True))
    # tables past the LDS room: the last rule is walked in global memory and decides on the last byte
    lines = []
    for i, ll in enumerate((12, 15, 16, 17, 24, 32, 33, 48, 100)):
        for last in (b"Z", b"Y"):
            for fix in (True, False):
                s = bytearray(_ab(i * 7 + 1, ll - 1))
                if fix:
                    s[-11], s[-9] = ord("a"), ord("b")                                # what the three rules look at: all three match with Z
                lines.append(apache_line(agent=bytes(s) + last))
    out.append(Chunk("tables past 48 KB, AND", [record(r, i) for i, r in enumerate(lines)], keep_time, list(BIG_TABLE_RULES) + [("regex", "time 2024")], "AND",
                     decide=True, big_tables=True))
    return out


@functools.lru_cache(maxsize=None)
def group(name):
    return {"staging": staging_chunks, "one_big": one_big_chunks, "full_batch": full_batch_chunks, "queue": queue_chunks, "tails": tail_chunks,
            "time_end": time_end_chunks, "fields": fields_chunks, "values": value_chunks, "rules": rules_chunks}[name]()


def all_chunks(names=GROUPS):
    return [(g, c) for g in names for c in group(g)]
