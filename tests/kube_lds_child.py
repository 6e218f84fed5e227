"""Child process of tests/test_kube_gpu.py: FLBGPU_KUBE_LDS_BLOB is read when a filter is created, so every budget gets a process of
its own.  argv: <budget> <pod blob bytes> <1 when the tail is expected in LDS>.  Builds the filter under the budget the environment
names, checks which path the layout reports, and compares the device with the CPU model on the alignment chunk and on a chunk of more
than one workgroup.  Prints "ok" and exits 0, or raises."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import flbamd_loader
import kube_model as km
from kube_chunks import alignment_chunk, blob_of, rows


def main():
    budget, nblob, in_lds = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3] == "1"
    assert os.environ.get("FLBGPU_KUBE_LDS_BLOB") == str(budget)
    g = flbamd_loader.load()
    g.init(0)
    props = [("merge_log", "on")]
    f, m = g.FilterKubernetes(props), km.Model(props)
    pod = blob_of(nblob)
    f.set_meta(pod, None)
    m.set_meta(pod, None)
    lay = f.layout()
    assert lay["tail_bytes"] == 11 + nblob and lay["in_lds"] == in_lds, lay
    for data in (alignment_chunk(), rows(300, stderr=(0, 63, 64, 299), plain=(1, 255, 256))):
        assert f.filter(data) == m.filter(data)
        assert f.counts() == m.counts() and f.counters() == m.counters() and f.counters()[3] == 0
    f.close()
    print("ok")


if __name__ == "__main__":
    main()
