"""The record builders of the filter_kubernetes tests and of tools/gen_kube_golden.py, kept apart so that the chunks can be built and
looked at without a device: cache entries of a chosen size, docker-JSON records, the chunk of n records with chosen streams, and
the seeded random configurations and records of the fuzz rounds."""
import json
import random
import struct

import synth
from checklist_chunks import GROUP_END, GROUP_START, R, f32, kv, rec, sv  # noqa: F401

BIG_T = R(b"\xcf" + struct.pack(">Q", 2 ** 33))          # a time the EventTime cannot hold
DOCKER_ID = "0123456789abcdef" * 4
STOCK_TAG = "kube.var.log.containers.apache-logs_default_apache-" + DOCKER_ID + ".log"


def blob_of(n):
    """one msgpack map of exactly n bytes"""
    if n == 1:
        return b"\x80"
    if n == 2:
        raise ValueError("no map of two bytes")
    if n == 3:
        return b"\x81\x00\x00"
    for key in ("k", "kk"):                               # 81, the key, a STR with its header
        room = n - 2 - len(key)
        for hdr in (1, 2, 3, 5):
            ln = room - hdr
            if ln >= 0 and hdr == len(synth.mp("x" * ln)) - ln:
                return b"\x81" + synth.mp(key) + synth.mp(("m%d-" % n + "x" * ln)[:ln])
    raise ValueError(n)


def pod_meta(labels=3, pad=0):
    """a pod map shaped like the reference's: pod_name, namespace_name, pod_id, labels, host, container_name, docker_id ..."""
    m = [("pod_name", "apache-logs"), ("namespace_name", "default"), ("pod_id", "e9f2963f-55f2-4c85-8d52-6a9a38e2a78c"),
         ("labels", kv(*[("label-%d" % i, "value-%d" % i) for i in range(labels)])), ("host", "node-1"), ("container_name", "apache"),
         ("docker_id", DOCKER_ID), ("container_image", "apache:2.4" + "x" * pad)]
    return synth.mp(kv(*m))


def docker(i, text, stream="stdout", sec=None):
    """a record as in_tail's docker parser leaves it: log, stream, time"""
    return rec(kv(("log", text), ("stream", stream), ("time", "2024-03-10T10:00:%02d.%09dZ" % (i % 60, i))), 1700000000 + i if sec is None else sec, i % 1000)


def json_line(i):
    return json.dumps({"level": "info", "msg": "request %d done\n" % i, "n": i, "ok": i % 2 == 0, "lat": i / 8.0}, separators=(",", ":"))


def rows(n, stderr=(), plain=()):
    """n docker records whose log is a JSON object, except the rows of `plain` (text); the rows of `stderr` come from that stream"""
    stderr, plain = set(stderr), set(plain)
    return b"".join(docker(i, "plain text %d\n" % i if i in plain else json_line(i), "stderr" if i in stderr else "stdout") for i in range(n))


def alignment_chunk():
    """records whose own part ends at every address mod 4: plain `log` values of 0 .. 7 bytes, kept as they are"""
    return b"".join(rec(kv(("log", "x" * ln)), 1 + ln) for ln in range(8)) + b"".join(rec(kv(("a", "y" * ln), ("log", '{"k":"%s"}' % ("z" * ln))), 20 + ln) for ln in range(8))


def nested(depth):
    """{"a": [[[ ... 1 ... ]]]} with `depth` arrays inside the object"""
    return '{"a":' + "[" * depth + "1" + "]" * depth + ',"b":"x"}'


LOGS = ['{"a":1}', '{"a":1} x', '{"a":1} 5', '{"a":1}{"b":2}', '[1]', 'plain', '', '  {"a":"x\\n"}  ', '{}', '{"s":"\\n"}', '{"s":"\\n\\n"}', '{"s":"x\\\\n"}',
        '{"s":"a\\\\n\\n\\\\r"}', '{"s":"\\\\n"}', '{"s":"n"}', '{"m":{"s":"x\\n"},"l":["y\\n"]}', '{"u":"end\\u000a"}', '{"d":0.1,"e":1e300,"f":123456789012345678901234567890}',
        '{"k":1,"k":2}', '{"x":"\\ud800"}', '{"z":"a\\u0000b"}', nested(7), nested(9), nested(31), nested(32), nested(33), nested(70),
        '{"a":' + "3." + "1" * 40 + '}', '{"t":"' + "x" * 30 + '\\n"}', '{"t":"' + "x" * 32 + '\\n"}', "{\"a\":\"caf\xc3\xa9 \\u00e9\"}", '{"a":', '{"a":1,}', 'null', '5']


def fuzz_round(seed):
    """(props, pod entry, namespace entry, chunk): a random configuration, random cache entries (a properties array with random
    excludes behind the pod's half of the time) and at most 2000 records whose `log` is drawn from every shape the merge knows"""
    rnd = random.Random(seed)
    props = []
    if rnd.random() < 0.8:
        props.append(("merge_log", rnd.choice(["on", "true", "yes"])))
    if rnd.random() < 0.5:
        props.append(("keep_log", rnd.choice(["off", "on"])))
    if rnd.random() < 0.4:
        props.append(("merge_log_trim", rnd.choice(["off", "on"])))
    if rnd.random() < 0.4:
        props.append(("merge_log_key", rnd.choice(["parsed", "", "k" * 40])))
    if rnd.random() < 0.3:
        props.append(("labels", "off"))
    pod = ns = None
    if rnd.random() < 0.85:
        pod = rnd.choice([pod_meta(), pod_meta(20, 300), blob_of(1), blob_of(rnd.randint(3, 70)), pod_meta(400, 9000)])
        if rnd.random() < 0.5:
            pod += b"\x94\xc0\xc0" + rnd.choice([b"\xc2\xc2", b"\xc3\xc2", b"\xc2\xc3", b"\xc3\xc3"])
    if rnd.random() < 0.4:
        ns = rnd.choice([blob_of(1), blob_of(rnd.randint(3, 40)), synth.mp(kv(("name", "default"), ("labels", kv(("team", "a")))))])
    odd_logs = [None, 7, -3, 2.5, True, R(b"\xc4\x03{} "), ["x"], kv(), kv(("in", "map\n"), ("n", 1)), R(b"\xdb\x00\x00\x00\x07{\"q\":1}"), sv(b'{"b":"\xff\xfe"}')]
    streams = ["stdout", "stderr", "std", "", "other", "stdout\0x", R(b"\xc4\x06stderr"), 5, None]
    recs = []
    n = rnd.choice([1, 63, 64, 65, 300, 1000, 2000])
    for i in range(n):
        pairs = []
        if rnd.random() < 0.9:
            r = rnd.random()
            log = json_line(i) if r < 0.5 else rnd.choice(LOGS) if r < 0.85 else rnd.choice(odd_logs)
            pairs.append((rnd.choice(["log", "log", "log", R(b"\xc4\x03log"), R(b"\xd9\x03log"), "logs", 3]), log))
        if rnd.random() < 0.8:
            pairs.append((rnd.choice(["stream", "stream", "s", "", "streams", "stream\0z", R(b"\xc4\x06stream")]), rnd.choice(streams)))
        if rnd.random() < 0.5:
            pairs.append(("time", "2024-03-10T10:00:00Z"))
        if rnd.random() < 0.2:
            pairs.append((R(b"\xda\x00\x02nc"), R(b"\xd3" + struct.pack(">q", 5))))      # non-canonical encodings in an untouched pair
        if rnd.random() < 0.1:
            pairs.append(("log", '{"second":1}'))
        rnd.shuffle(pairs)
        if rnd.random() < 0.02:
            recs.append(GROUP_START if rnd.random() < 0.5 else GROUP_END)
        t = rnd.random()
        if t < 0.05:
            recs.append(synth.mp([1700000000 + i, kv(*pairs)]))
        elif t < 0.1:
            recs.append(synth.mp([1700000000.25 + i, kv(*pairs)]))
        else:
            recs.append(rec(kv(*pairs), 1700000000 + i, i, kv(("m", i)) if rnd.random() < 0.1 else None))
    return props, pod, ns, b"".join(recs)
