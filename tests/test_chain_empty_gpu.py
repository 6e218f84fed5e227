"""flb_filter_do's rule "an empty MODIFIED output ends the chain" (src/flb_filter.c:247-269) through each of the three arms of the chain
(flbgpu.cpp chain_dev): the fused parser + grep pair, two filter_grep instances as one pass, and the filters one by one.  Three-filter
chains whose first stage or pair drops every record, with a filter_modify behind them that would change every record it got: the
chain answers MODIFIED with an empty output, the stages that ran report what their one-by-one calls report, the stages behind report
nothing."""
import pytest
import flbamd_loader
import synth
from test_grep_pair_gpu import _upload

pytestmark = pytest.mark.gpu

APACHE2 = (r'^(?<host>[^ ]*) [^ ]* (?<user>[^ ]*) \[(?<time>[^\]]*)\] "(?<method>\S+)(?: +(?<path>[^ ]*) +\S*)?" '
           r'(?<code>[^ ]*) (?<size>[^ ]*)(?: "(?<referer>[^\"]*)" "(?<agent>.*)")?$')
TIME_FMT = "%d/%b/%Y:%H:%M:%S %z"
N = 64
SET = [("Set", "k x")]
ZERO = dict(ret=0, in_records=0, out_records=0, out_bytes=0)


@pytest.fixture(scope="module")
def g():
    m = flbamd_loader.load()
    m.init(0)
    return m


@pytest.fixture(scope="module")
def records():
    data, off, ep = synth.apache_records(N)
    return [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(N)]


@pytest.fixture(scope="module")
def blob(records):
    return b"".join(records)


def _parser_chain(g):
    p = g.Parser(APACHE2, time_fmt=TIME_FMT, time_key="time")
    return [g.FilterParser("log", [p]), g.FilterGrep([("regex", "code ^nomatch$")]), g.FilterModify(SET)]


def _grep_first_drops(g):
    return [g.FilterGrep([("regex", "log ^nomatch$")]), g.FilterGrep([("regex", "log .")]), g.FilterModify(SET)]


def _grep_second_drops(g):
    return [g.FilterGrep([("regex", "log .")]), g.FilterGrep([("regex", "log ^nomatch$")]), g.FilterModify(SET)]


CHAINS = {"parser_grep": _parser_chain, "grep_first_drops": _grep_first_drops, "grep_second_drops": _grep_second_drops}
_one_by_one = {}


def one_by_one(g, name, blob):
    """what fresh instances report when the caller hands the chunk from one to the next (flbgpu_filter_run: no chain, no pair)"""
    if name not in _one_by_one:
        filters = CHAINS[name](g)
        stats, cur, ended = [], blob, False
        for f in filters:
            if ended:
                stats.append(dict(ZERO))
                continue
            ret, out = f.filter(cur)
            i, o = f.counts()
            mod = ret == g.MODIFIED
            stats.append(dict(ret=ret, in_records=i, out_records=o if mod else i, out_bytes=len(out) if mod else len(cur)))
            if mod:
                cur = out
                ended = len(out) == 0
        for f in filters:
            f.close()
        _one_by_one[name] = stats
    return _one_by_one[name]


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "no_spec"])
@pytest.mark.parametrize("fuse", [True, False], ids=["pairs", "no_fuse"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_empty_output_ends_the_chain(g, records, blob, monkeypatch, name, fuse, ahead):
    want = one_by_one(g, name, blob)
    # the stage or pair in front drops everything and the chain ends there: nothing reaches filter_modify
    dropper = 0 if name == "grep_first_drops" else 1
    assert want[dropper]["ret"] == g.MODIFIED and want[dropper]["in_records"] == N and want[dropper]["out_records"] == 0
    assert want[dropper]["out_bytes"] == 0 and want[dropper + 1:] == [ZERO] * (2 - dropper)
    if dropper == 1:
        assert want[0]["in_records"] == want[0]["out_records"] == N
    # both switches are read per call: the parser + grep pair (off: one by one), the launch ahead of the sizes that a small chunk
    # takes (on: two filter_grep instances run one by one; off: as one pass)
    if not fuse:
        monkeypatch.setenv("FLBGPU_NO_FUSE", "1")
    if not ahead:
        monkeypatch.setenv("FLBGPU_NO_SPEC", "1")
    filters = CHAINS[name](g)
    for f in filters:
        f.profile(True)
    ch = g.FilterChain(filters)
    # host-level call
    assert ch.filter(blob) == (g.MODIFIED, b"")
    host_stats = ch.last_stats()
    print(name, fuse, ahead, host_stats, [sorted(f.profile_read()) for f in filters])
    assert host_stats == want
    # device-level call
    chunk, bufs, _ = _upload(g, records)
    ret, out = ch.filter_dev(chunk)
    assert ret == g.MODIFIED and int(out.bytes) == 0
    assert ch.last_stats() == want
    prof = [f.profile_read() for f in filters]
    assert prof[2] == {}, "filter_modify ran behind an empty output"
    if name == "parser_grep":
        # the fused pair never writes the parsed chunk and never runs grep's own kernels
        assert ("k_parser_emit" not in prof[0] and prof[1] == {}) == fuse, prof
    elif name == "grep_first_drops":
        assert prof[1] == {}, "the second filter_grep ran behind an empty output"
    if name != "parser_grep":
        assert ("k_grep_lane(two instances)" in prof[0]) == (not ahead), prof
    for f in filters:
        f.close()
    L = g.lib()
    L.flbgpu_dev_free(bufs[0]); L.flbgpu_dev_free(bufs[1])


def test_the_third_filter_would_modify(g, blob):
    f = g.FilterModify(SET)
    ret, out = f.filter(blob)
    assert ret == g.MODIFIED and f.counts() == (N, N) and len(out) > len(blob)
    f.close()
