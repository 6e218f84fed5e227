"""filter_checklist's configuration and list loader on the host (csrc/checklist.cpp flbgpu_checklist_parse_check, no device needed)
against the CPU model's restatement of the config map, init_config and load_file_patterns (tests/checklist_model.py): every recorded
configuration with its list file, the refusals, and the loader's edges."""
import base64
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flbamd_loader
import checklist_model as cm
from checklist_chunks import LIST, MISSING

CASES = json.load(open(os.path.join(HERE, "golden", "checklist_ref_cases.json")))["cases"]
RAN_BUT_REFUSED = {"ld_nul_at_line_start"}


@pytest.fixture(scope="module")
def g():
    return flbamd_loader.load()


def on_disk(props, lst, tmp_path):
    """the properties with the list written to a file of tmp_path"""
    path = str(tmp_path / "list.txt")
    if lst is not None:
        with open(path, "wb") as f:
            f.write(lst)
    sub = {LIST: path, MISSING: str(tmp_path / "no_such_file")}
    return [(k, sub.get(v, v)) for k, v in props]


def product(g, props):
    try:
        return g.checklist_parse_check(props)
    except ValueError:
        return None


def model(props):
    try:
        return cm.describe(cm.parse(props))
    except ValueError:
        return None


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_configurations(g, case, tmp_path):
    props = on_disk([tuple(p) for p in case["props"]], base64.b64decode(case["list"]) if case["list"] is not None else None, tmp_path)
    want = model(props)
    # where the real plugin did not start, or died, create refuses -- and at the one list the reference reads out of bounds on
    assert (want is None) == bool(case.get("refused") or case.get("crashed") or case["name"] in RAN_BUT_REFUSED)
    assert product(g, props) == want
    if want is None:
        assert g.last_error().startswith("filter_checklist: ")


def test_the_line_says_what_was_loaded(g, tmp_path):
    props = on_disk([("file", LIST), ("lookup_key", "$m['a'][2]"), ("mode", "PARTIAL"), ("ignore_case", "yes"), ("record", "k v w"),
                     ("record", "t TRUE"), ("record", "n null"), ("record", "f False")], b"Ab\n#c\n\nCD\r\n", tmp_path)
    assert g.checklist_parse_check(props) == ("mode=partial;fold=1;key=K6d.61[2];records=K6b:s77,K74:t,K6e:n,K66:f;entries=2;slots=0;load=ok;digest=%016x"
                                              % cm.digest([b"ab", b"cd"])) == model(props)
    assert g.checklist_parse_check([]) == "mode=exact;fold=0;key=K6c6f67;records=;entries=0;slots=1;load=no file;digest=cbf29ce484222325"
    assert "load=cannot open" in g.checklist_parse_check(on_disk([("file", MISSING)], None, tmp_path))
    assert "key=-;" in g.checklist_parse_check([("lookup_key", "$TAG")])


LISTS = [
    b"", b"\n", b"a", b"a\n", b"a\r\n", b"a\r", b"\r\n", b"\r", b"#\n", b" #x\n", b"a\n\nb\n", b"a\0b\n", b"a\0b", b"a\nb\0c\nd\n", b"a\n\0", b"\0",
    b"a\n\0b\n", b"x" * 2044 + b"\r\n" + b"y\n", b"x" * 2045 + b"\r\n" + b"y\n", b"x" * 2045 + b"\ny\n", b"x" * 2046 + b"\ny\n", b"x" * 2046,
    b"x" * 2045, b"a\n" + b"x" * 2046, b"a\n" + b"x" * 2047 + b"\n", b"x" * 5000 + b"\n", b"A\xc9Z\n", b"%\n_\n",
]


@pytest.mark.parametrize("i", range(len(LISTS)))
@pytest.mark.parametrize("fold", ["off", "on"])
def test_loader_edges(g, tmp_path, i, fold):
    props = on_disk([("file", LIST), ("ignore_case", fold)], LISTS[i], tmp_path)
    assert product(g, props) == model(props)


def test_what_the_loader_edges_decide(tmp_path):
    def m(lst):
        try:
            c = cm.parse([("file", b"f")], {b"f": lst})
            return c.entries, c.status, c.stop_line
        except ValueError:
            return None
    assert m(b"a\r") == ([b"a\r"], cm.OK, 0) and m(b"\r\n") == ([], cm.OK, 0) and m(b"\r") == ([b"\r"], cm.OK, 0)
    assert m(b"a\n\0") is None and m(b"\0") is None and m(b"a\n\0b\n") is None
    assert m(b"a\nb\0c\nd\n") == ([b"a"], cm.STOPPED, 1) and m(b"a\0b") == ([b"a"], cm.OK, 0)
    # 2045 bytes and a "\r\n": the piece is cut in front of the '\n', which then is a line of its own
    assert m(b"x" * 2045 + b"\r\ny\n") == ([], cm.STOPPED, 0)
    assert m(b"x" * 2044 + b"\r\ny\n") == ([b"x" * 2044, b"y"], cm.OK, 0)
    assert m(b"x" * 2046) == ([], cm.STOPPED, 0) and m(b"x" * 2045) == ([b"x" * 2045], cm.OK, 0)


REFUSED = [
    [("record", "only")], [("record", "")], [("nope", "1")], [("ignore_case", "2")], [("print_query_time", "")], [("mode", "exact"), ("MODE", "exact")],
    [("file", "a"), ("file", "a")], [("lookup_key", "$a['x")], [("lookup_key", "$a[x]")], [("lookup_key", "${HOME}")], [("lookup_key", "k" * 128)],
    [("record", "k%d v" % i) for i in range(65)], [("record", "k " + "v" * 32768)],
]
STARTS = [
    [("record", "k%d v" % i) for i in range(64)], [("lookup_key", "k" * 127)], [("mode", "")], [("lookup_key", "")], [("lookup_key", "$")],
    [("lookup_key", "a.b")], [("lookup_key", "$a.b")], [("record", "k " + "v" * 30000)],
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_refused(g, i):
    assert product(g, REFUSED[i]) is None and model(REFUSED[i]) is None


@pytest.mark.parametrize("i", range(len(STARTS)))
def test_starts(g, i):
    assert product(g, STARTS[i]) == model(STARTS[i]) is not None


def table_props(nbytes):
    """one `record` whose table is exactly nbytes: 16 + 16 bytes of words, the 4-byte key "log", a 4-byte record key, its STR header
    and a value behind a 3-byte STR header"""
    return [("record", "abcd " + "v" * (nbytes - 32 - 4 - 4 - 5 - 3))]


def test_table_limit(g):
    for n in (32768, 32766):
        p = table_props(n)
        assert cm.table_bytes(cm.parse(p)) == 32768
    assert product(g, table_props(32768)) == model(table_props(32768)) is not None
    assert product(g, table_props(32769)) is None and model(table_props(32769)) is None
    assert "32768" in g.last_error()


def test_dense_switch_shows_in_the_slot_count(g, tmp_path, monkeypatch):
    props = on_disk([("file", LIST)], b"".join(b"e%d\n" % i for i in range(100)), tmp_path)
    assert ";slots=256;" in g.checklist_parse_check(props)
    monkeypatch.setenv("FLBGPU_CHECKLIST_DENSE", "1")
    assert ";slots=128;" in g.checklist_parse_check(props) and g.checklist_parse_check(props) == cm.describe(cm.parse(props), dense=True)
    for n, slots in ((0, 1), (1, 2), (127, 128), (128, 256)):
        p = on_disk([("file", LIST)], b"".join(b"e%d\n" % i for i in range(n)), tmp_path)
        assert ";slots=%d;" % slots in g.checklist_parse_check(p)
