"""The CPU model's partial match (tests/checklist_model.py like(): SQLite's patternCompare restated) against SQLite itself, through
Python's sqlite3 with this project's own statement: the edge list and 20 000 seeded random pairs over a small alphabet."""
import os
import random
import sqlite3
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import checklist_model as cm
from checklist_chunks import LIKE_EDGES

STATEMENT = "SELECT CAST(?1 AS TEXT) LIKE (CAST(?2 AS TEXT) || '%')"
ALPHABET = [b"a", b"b", b"A", b"%", b"_", b"\x00", b"\x80", b"\xa9", b"\xc0", b"\xc3", b"\xe2", b"\xf0", b"\xff"]
ENTRY_ALPHABET = [c for c in ALPHABET if c != b"\x00"]        # a loaded entry is cut at strlen: it never holds a NUL
SEED, PAIRS, MAXLEN = 20301, 20000, 12


@pytest.fixture(scope="module")
def db():
    con = sqlite3.connect(":memory:")
    con.execute("PRAGMA case_sensitive_like = true")
    yield con
    con.close()


def sqlite_like(db, value, entry):
    # the plugin binds the value with its length and the list holds entries cut at strlen: an entry has no NUL
    return bool(db.execute(STATEMENT, (bytes(value), bytes(entry))).fetchone()[0])


@pytest.mark.parametrize("i", range(len(LIKE_EDGES)))
def test_edges(db, i):
    value, entry, want = LIKE_EDGES[i]
    assert sqlite_like(db, value, entry) == want
    assert cm.like(value, entry) == want


def test_random_pairs(db):
    rnd = random.Random(SEED)
    yes = no = 0
    for _ in range(PAIRS):
        value = b"".join(rnd.choice(ALPHABET) for _ in range(rnd.randint(0, MAXLEN)))
        entry = b"".join(rnd.choice(ENTRY_ALPHABET) for _ in range(rnd.randint(0, MAXLEN)))
        want = sqlite_like(db, value, entry)
        assert cm.like(value, entry) == want, (value, entry, want)
        yes += want
        no += not want
    assert yes + no == PAIRS and yes >= PAIRS // 10 and no >= PAIRS // 10, (yes, no)
