"""Child process of tests/test_lane_stride_gpu.py: FLBGPU_LANE_MAX_BLOCKS is read once per process, so every cap gets a process of its
own.  argv: `host` -- no GPU work: what the environment holds must leave the default of 65536 blocks; or <cap> <filter> -- the cap
must be the one the environment names (0: none), then the filter (tests/filter_paths.py) takes 1025 records against its CPU model: all good,
and with the undecodable record as the lone lane of the last trip (row 1024) and on either side of a trip boundary (rows 512, 511),
after each the all-good chunk again on the same object.  Prints "ok" and exits 0, or raises."""
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import flbamd_loader
from filter_paths import BAD, good, make, same
import synth

N = 1025


def main():
    g = flbamd_loader.load()
    if sys.argv[1] == "host":
        assert g.lib().flbgpu_lane_max_blocks() == 65536, os.environ.get("FLBGPU_LANE_MAX_BLOCKS")
        print("ok")
        return
    cap, name = int(sys.argv[1]), sys.argv[2]
    if cap:
        assert g.lib().flbgpu_lane_max_blocks() == cap
    g.init(0)
    rows = [good(i) for i in range(N)]
    all_good = b"".join(rows)
    with tempfile.TemporaryDirectory() as tmp:
        f, m = make(g, name, pathlib.Path(tmp))
        try:
            for bad in (None, 1024, 512, 511):
                data = all_good if bad is None else b"".join(rows[:bad]) + BAD + b"".join(rows[bad + 1:])
                same(name, f, m, data)
                ret, out = same(name, f, m, all_good)
                assert ret == g.MODIFIED and f.counts()[0] == N
                assert len(synth.unpack_all(out)) == (0 if name == "rewrite_tag" else N)
        finally:
            f.close()
    print("ok")


if __name__ == "__main__":
    main()
