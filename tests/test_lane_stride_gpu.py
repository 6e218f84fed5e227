"""The grid-stride trips of the lane-per-record kernels (csrc/lane_rows.inc): a launch gets at most 65536 blocks, so only a chunk of
more than 16.7 M records makes a block walk a second stretch of rows.  The test switch FLBGPU_LANE_MAX_BLOCKS lowers the cap: under
cap 2 a chunk of 1025 records is three trips of the 256-lane kernels (the last one holds one live lane in one wave, every other wave
has left the loop) and nine of modify's 64-lane blocks, under cap 1 five and seventeen.  The switch is read once per process, so
tests/lane_stride_child.py does the work in a fresh process per cap; cap 0 is the same chunks without the switch."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from filter_paths import FILTERS

pytestmark = pytest.mark.gpu
CHILD = os.path.join(HERE, "lane_stride_child.py")


def child(args, value):
    env = dict(os.environ)
    env.pop("FLBGPU_LANE_MAX_BLOCKS", None)
    if value is not None:
        env["FLBGPU_LANE_MAX_BLOCKS"] = value
    r = subprocess.run([sys.executable, CHILD] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().strip().endswith("ok"), r.stderr.decode()[-800:]


@pytest.mark.parametrize("cap", [0, 2, 1], ids=["nocap", "cap2", "cap1"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_stride_trips(name, cap):
    child([str(cap), name], str(cap) if cap else None)


@pytest.mark.parametrize("value", [None, "", "0", "-1", "abc", "65537", "2x", "65536"])
def test_switch_values_that_leave_the_default(value):
    child(["host"], value)
